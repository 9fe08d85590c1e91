"""Register audit of the per-gene thresholds translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel in it -- the five of csrc/thresholds.hip and the rocprim sort kernels it
instantiates -- may use scratch memory."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("thresholds_keys_kernel", "thresholds_segments_kernel", "thresholds_chunks_kernel", "thresholds_genes_kernel",
           "thresholds_absent_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/thresholds.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "thresholds.s"]


def test_thresholds_kernels_use_no_scratch(rows):
    own = {r["name"].split("(")[0] for r in rows if r["name"].startswith("thresholds_")}
    assert own == set(KERNELS), sorted(own)
    assert len(rows) > len(KERNELS)                                  # the library kernels of the sort are in the table too
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
