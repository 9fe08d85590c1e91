"""Register audit of the polygon-overlap translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of polygon_overlap.s may use scratch memory, and the LDS per workgroup is what
DESIGN 3.5n states -- none on the register tier, two rings of 16 B a vertex at 256 vertices (8192 B) on the small tier and
at 4096 vertices (131072 B, one workgroup per CU) on the large one."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the scan is post_common.h's counts_to_offsets_kernel (once ov_scan_kernel), still one instance per type: 9 rows as before
KERNELS = ("ov_bin_kernel", "counts_to_offsets_kernel", "ov_grid_kernel", "ov_cand_kernel", "ov_pair_reg_kernel", "ov_pair_lds_kernel")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/polygon_overlap.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "polygon_overlap.s"]


def test_overlap_kernels_use_no_scratch_and_the_stated_lds(rows):
    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1]
    assert sorted({short(r) for r in rows}) == sorted(KERNELS)
    assert len(rows) == 9                                            # scan per type, candidates count / fill, LDS pairs per tier
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = {(short(r), "<256>" in r["name"]): r["lds"] for r in rows}
    assert lds[("ov_pair_reg_kernel", False)] == 0
    assert lds[("ov_pair_lds_kernel", True)] == 2 * 256 * 16 == 8192
    assert lds[("ov_pair_lds_kernel", False)] == 2 * 4096 * 16 == 131072
    assert LDS_PER_CU // lds[("ov_pair_lds_kernel", False)] == 1 and LDS_PER_CU // lds[("ov_pair_lds_kernel", True)] >= 16
    assert lds[("ov_bin_kernel", False)] == 0 and lds[("ov_grid_kernel", False)] == 0 and lds[("ov_cand_kernel", False)] == 0
    assert lds[("counts_to_offsets_kernel", False)] <= 2048
