"""Register audit of the contamination translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: the kernels of csrc/contamination.hip are exactly the frequency kernel and the two
instances of the posterior kernel (table in LDS / through L2), and none of them uses scratch memory."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("neighbor_frequencies_kernel", "contamination_posterior_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: a few seconds
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/contamination.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "contamination.s"]


def test_contamination_kernels_use_no_scratch(rows):
    names = [r["name"] for r in rows]
    assert {n.split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1] for n in names} == set(KERNELS), sorted(names)
    assert len(rows) == 1 + 2
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
