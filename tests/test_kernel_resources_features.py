"""Register audit of the features translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of csrc/features.hip -- the Gram, its reduction and the eight instances of
the projection (1..4 column chunks x float32 / float64 output) -- may use scratch memory, and the Gram is the float64
MFMA it claims to be."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("features_gram_kernel", "features_gram_reduce_kernel", "features_project_kernel")
ASM = os.path.join(ROOT, "build", "asm", "features.s")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: a few seconds
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/features.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "features.s"]


def test_features_kernels_use_no_scratch(rows):
    names = [r["name"] for r in rows]
    assert {n.split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1] for n in names} == set(KERNELS), sorted(names)
    assert len(rows) == 2 + 8
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled


def test_gram_is_a_float64_mfma(rows):
    with open(ASM) as f:
        text = f.read()
    assert text.count("v_mfma_f64_16x16x4_f64") >= 4                  # one per 16-gene block of the second tile, at least
