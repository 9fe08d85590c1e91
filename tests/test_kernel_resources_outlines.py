"""Register audit of the concave outline translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel in it -- its own two, the front and back end it shares with boundaries.hip
through cell_rings.h, and the rocprim sort and select kernels it instantiates -- may use scratch memory, and the per-cell
state takes the LDS the header documents: 68 bytes per point of capacity."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("bnd_keys_kernel", "out_bin_kernel", "out_cell_kernel", "bnd_scan_kernel", "bnd_emit_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/outlines.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "outlines.s"]


def test_outlines_kernels_use_no_scratch_and_the_documented_lds(rows):
    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1]
    own = [short(r) for r in rows if "bnd_" in r["name"].split("(")[0] or "out_" in r["name"].split("(")[0]]
    assert set(own) == set(KERNELS), sorted(own)
    assert len(own) == len(KERNELS) + 6 + 1                          # emit: smoothing 0 .. 6; the cell kernel: two capacities
    assert len(rows) > len(own)                                      # the library kernels of the sort are in the table too
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = sorted(r["lds"] for r in rows if short(r) == "out_cell_kernel")
    assert lds == [68 * 256, 68 * 2048] and lds[1] <= 160 * 1024
