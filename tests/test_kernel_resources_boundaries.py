"""Register audit of the cell boundary translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel in it -- the seven of csrc/boundaries.hip (the emit kernel in one instance per
number of Chaikin iterations) and the rocprim sort and select kernels it instantiates -- may use scratch memory."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("bnd_keys_kernel", "bnd_bin_kernel", "bnd_short_kernel", "bnd_long_kernel", "bnd_chunk_kernel", "bnd_scan_kernel",
           "bnd_emit_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/boundaries.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "boundaries.s"]


def test_boundaries_kernels_use_no_scratch(rows):
    own = [r["name"].split("(")[0].split("<")[0].split(" ")[-1] for r in rows if "bnd_" in r["name"].split("(")[0]]
    assert set(own) == set(KERNELS), sorted(own)
    assert len(own) == len(KERNELS) + 6                              # emit: smoothing 0 .. 6
    assert len(rows) > len(own)                                      # the library kernels of the sort are in the table too
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = {r["name"].split("(")[0]: r["lds"] for r in rows if "bnd_" in r["name"].split("(")[0]}
    assert lds["bnd_long_kernel"] == lds["bnd_chunk_kernel"] == 65536
