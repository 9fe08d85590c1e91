"""Register audit of the optimizer translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: the gradient guard's kernels and the guarded update use no scratch memory, and the plain
update -- now one instantiation of the template the guarded one shares -- has exactly the registers it had before the
guard existed (recorded from the commit before: 50 VGPRs, 75 SGPRs, no scratch, no LDS; its instruction stream compared
equal too, label numbers aside).  The guarded update costs one SGPR more (the state pointer) and no VGPR."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("adam_advance_kernel", "adam_advance_guarded_kernel", "adam_kernel", "grad_guard_partial_kernel",
           "grad_guard_finish_kernel")


def short(r):
    return r["name"].split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1]


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: seconds
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/adam.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "adam.s"]


def test_no_kernel_of_the_unit_uses_scratch(rows):
    assert sorted({short(r) for r in rows}) == sorted(KERNELS), sorted({short(r) for r in rows})
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = {}
    for r in rows:
        lds.setdefault(short(r), []).append(r["lds"])
    assert lds["grad_guard_partial_kernel"] == [48]                   # 4 wave sums (8 bytes) + 4 wave flags (4 bytes)
    assert lds["grad_guard_finish_kernel"] == [56]                    # the same + the skip word (padded to 8)
    assert lds["adam_kernel"] == [0, 0] and lds["adam_advance_kernel"] == lds["adam_advance_guarded_kernel"] == [0]


def test_plain_update_keeps_its_registers_and_the_guarded_one_adds_no_vgpr(rows):
    update = {("guard" in r["name"]): r for r in rows if short(r) == "adam_kernel"}
    assert set(update) == {False, True}
    plain, guarded = update[False], update[True]
    assert plain["name"].endswith("adam_kernel<>(AdamBatch)"), plain["name"]          # no guard argument at all
    assert (plain["vgpr"], plain["sgpr"], plain["scratch"], plain["lds"]) == (50, 75, 0, 0)
    assert (guarded["vgpr"], guarded["sgpr"], guarded["scratch"], guarded["lds"]) == (50, 76, 0, 0)
    advance = [r for r in rows if short(r) == "adam_advance_kernel"][0]
    assert (advance["vgpr"], advance["sgpr"], advance["scratch"]) == (6, 5, 0)
