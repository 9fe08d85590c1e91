"""Register audit of the ring-simplification translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of simplify.s may use scratch memory, and the LDS per workgroup is what
DESIGN 3.5m states -- the ring (16 B a vertex), the kept list and pending stack (2 B) and the keep mask (1 B) for the mark
kernel, the ring alone for the validity kernel, at 256 vertices in the small tier and 4096 in the large."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("sr_bin_kernel", "sr_mark_kernel", "sr_scan_kernel", "sr_emit_kernel", "sr_valid_kernel")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/simplify.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "simplify.s"]


def test_simplify_kernels_use_no_scratch_and_the_stated_lds(rows):
    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1]
    assert sorted({short(r) for r in rows}) == sorted(KERNELS)
    assert len(rows) == 7                                            # mark and valid once per tier
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = {(short(r), "<256>" in r["name"]): r["lds"] for r in rows}
    assert lds[("sr_mark_kernel", True)] == 256 * (16 + 2 + 1) == 4864
    assert lds[("sr_mark_kernel", False)] == 4096 * (16 + 2 + 1) == 77824
    assert lds[("sr_valid_kernel", True)] == 256 * 16 and lds[("sr_valid_kernel", False)] == 4096 * 16
    assert LDS_PER_CU // lds[("sr_mark_kernel", False)] == 2 and LDS_PER_CU // lds[("sr_valid_kernel", False)] == 2
    assert LDS_PER_CU // lds[("sr_mark_kernel", True)] >= 32         # the small tier: LDS never limits the waves of a CU
    assert lds[("sr_bin_kernel", False)] == 0 and lds[("sr_emit_kernel", False)] == 0 and lds[("sr_scan_kernel", False)] <= 2048
