"""Register audit of the ring-repair translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of repair.s may use scratch memory, and the LDS per workgroup of the sort kernel
is what DESIGN 3.5o states -- the differences (16 B a vertex) and the index (2 B), at 256 vertices in the small tier and
4096 in the large."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("rr_copy_kernel", "rr_bin_kernel", "rr_sort_kernel")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/repair.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "repair.s"]


def test_repair_kernels_use_no_scratch_and_the_stated_lds(rows):
    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1]
    assert sorted({short(r) for r in rows}) == sorted(KERNELS)
    assert len(rows) == 4                                            # the sort once per tier
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = {(short(r), "<256>" in r["name"]): r["lds"] for r in rows}
    assert lds[("rr_sort_kernel", True)] == 256 * (16 + 2) == 4608
    assert lds[("rr_sort_kernel", False)] == 4096 * (16 + 2) == 73728
    assert LDS_PER_CU // lds[("rr_sort_kernel", False)] == 2         # two large-tier workgroups a CU
    assert LDS_PER_CU // lds[("rr_sort_kernel", True)] >= 32         # the small tier: LDS never limits the waves of a CU
    assert lds[("rr_copy_kernel", False)] == 0 and lds[("rr_bin_kernel", False)] == 0
