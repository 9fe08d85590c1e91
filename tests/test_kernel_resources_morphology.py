"""Register audit of the morphology translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: the kernels of csrc/morphology.hip are the binning kernel and the two polygon kernels
(register route, LDS route), and none of them uses scratch memory."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("morph_bin_kernel", "morph_short_kernel", "morph_long_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: a few seconds
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/morphology.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "morphology.s"]


def test_morphology_kernels_use_no_scratch(rows):
    names = [r["name"] for r in rows]
    assert {n.split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1] for n in names} == set(KERNELS), sorted(names)
    assert len(rows) == 3
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
