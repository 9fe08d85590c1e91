"""Register audit of the two loss-head translation units (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads.  The ordered route's kernels -- and the radix sort instantiated beside them -- use no
scratch memory at any storage type and width; the chained route's kernels, whose shared pieces moved into loss_head.h, have
exactly the registers they had before the ordered route existed (recorded from the commit before; the instruction stream of
loss_head.s compared equal too)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (vgpr, sgpr, lds) of loss_head_fwd_kernel / loss_head_bwd_kernel <T, CPL> on the commit before, T in the order the
# dispatcher instantiates them (float, bf16, f16), CPL = 2, 4, 8
BEFORE = {"loss_head_bwd_kernel": [(57, 84, 28), (68, 84, 28), (86, 84, 28), (55, 84, 28), (64, 80, 28), (95, 80, 28),
                                   (57, 84, 28), (64, 80, 28), (90, 84, 28)],
          "loss_head_fwd_kernel": [(58, 58, 16), (58, 58, 16), (58, 60, 16), (58, 58, 16), (58, 58, 16), (66, 60, 16),
                                   (58, 58, 16), (58, 58, 16), (62, 60, 16)],
          "loss_head_finish_kernel": [(12, 27, 28)]}
ORDERED = ("loss_head_keys_kernel", "loss_head_offsets_kernel", "loss_head_ordered_bwd_kernel")


def short(r):
    return r["name"].split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1]


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # two translation units: a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/loss_head.s",
                        "../../build/asm/loss_head_ordered.s"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] in ("loss_head.s", "loss_head_ordered.s")]


def test_the_ordered_route_uses_no_scratch(rows):
    mine = [r for r in rows if r["file"] == "loss_head_ordered.s"]
    found = {}
    for r in mine:
        found.setdefault(short(r), []).append(r)
    for name in ORDERED:
        assert name in found, (name, sorted(found))
    assert len(found["loss_head_keys_kernel"]) == len(found["loss_head_ordered_bwd_kernel"]) == 9      # 3 types x 3 widths
    spilled = {r["name"][:120]: r["scratch"] for r in mine if r["scratch"]}                           # the sort's kernels too
    assert not spilled, spilled
    # the backward's LDS: 16 partial sums of C floats + the deferred finish's 7 words; two blocks a SIMD at least
    assert sorted(r["lds"] for r in found["loss_head_ordered_bwd_kernel"]) == sorted([2048 + 28, 4096 + 28, 8192 + 28] * 3)
    assert max(r["vgpr"] for r in found["loss_head_ordered_bwd_kernel"]) <= 128
    assert all(r["lds"] == 0 for r in found["loss_head_keys_kernel"] + found["loss_head_offsets_kernel"])


def test_the_chained_route_keeps_its_registers(rows):
    old = [r for r in rows if r["file"] == "loss_head.s"]
    got = {}
    for r in old:
        assert r["scratch"] == 0, r["name"][:120]
        got.setdefault(short(r), []).append((r["vgpr"], r["sgpr"], r["lds"]))
    assert set(got) == set(BEFORE), sorted(got)
    for name, want in BEFORE.items():
        assert sorted(got[name]) == sorted(want), (name, got[name])
