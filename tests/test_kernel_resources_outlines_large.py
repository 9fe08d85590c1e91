"""Register audit of the large-cell outline translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel in it -- its own, outline_cell.h's two, the front and back end of cell_rings.h, and
the rocprim sort and select kernels it instantiates -- may use scratch memory; the LDS routes take what outlines.hip's take, and the
large-cell kernel keeps its state in the workspace: a few hundred bytes of LDS for its reductions."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("bnd_keys_kernel", "out_bin_kernel", "out_cell_kernel", "outl_large_kernel", "bnd_scan_kernel", "bnd_emit_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/outlines_large.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "outlines_large.s"]


def test_large_outline_kernels_use_no_scratch_and_little_lds(rows):
    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1]
    own = [short(r) for r in rows if any(p in r["name"].split("(")[0] for p in ("bnd_", "out_", "outl_"))]
    assert set(own) == set(KERNELS), sorted(own)
    assert len(own) == len(KERNELS) + 6 + 1                          # emit: smoothing 0 .. 6; the LDS kernel: two capacities
    assert len(rows) > len(own)                                      # the library kernels of the sort are in the table too
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    assert sorted(r["lds"] for r in rows if short(r) == "out_cell_kernel") == [68 * 256, 68 * 2048]
    large = [r for r in rows if short(r) == "outl_large_kernel"]
    assert len(large) == 1 and large[0]["lds"] <= 1024
