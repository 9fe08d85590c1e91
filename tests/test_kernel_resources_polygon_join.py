"""Register audit of the polygon join translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel in it -- the six of csrc/polygon_join.hip (the two polygon kernels in a count
and a fill instance each) and the rocprim sort kernels it instantiates -- may use scratch memory."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the scan is post_common.h's counts_to_offsets_kernel (once pjoin_scan_kernel): same count of rows, one other name
KERNELS = ("pjoin_keys_kernel", "pjoin_cells_kernel", "pjoin_bin_kernel", "pjoin_short_kernel", "pjoin_long_kernel",
           "counts_to_offsets_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/polygon_join.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "polygon_join.s"]


def test_polygon_join_kernels_use_no_scratch(rows):
    own = [r["name"].split("(")[0].split("<")[0].split(" ")[-1] for r in rows if "pjoin_" in r["name"].split("(")[0] or "counts_to_offsets_" in r["name"].split("(")[0]]
    assert set(own) == set(KERNELS), sorted(own)
    assert len(own) == len(KERNELS) + 2                              # short and long: a count and a fill instance each
    assert len(rows) > len(own)                                      # the library kernels of the sort are in the table too
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
