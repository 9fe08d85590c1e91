"""Register audit of the phenograph translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of csrc/phenograph.hip -- the norms, the four instances of the fused
product-and-selection kernel (d padded to 32 / 64 / 128 / 256), the finish pass, the Jaccard merge and the four Louvain
kernels -- may use scratch memory, and the kNN is the fp32 MFMA it claims to be."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("knn_norm_kernel", "knn_select_kernel", "knn_finish_kernel", "jaccard_kernel", "louvain_move_kernel",
           "louvain_apply_kernel", "louvain_internal_kernel", "louvain_modularity_kernel")
ASM = os.path.join(ROOT, "build", "asm", "phenograph.s")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: a few seconds
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/phenograph.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "phenograph.s"]


def test_phenograph_kernels_use_no_scratch(rows):
    names = [r["name"] for r in rows]
    assert {n.split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1] for n in names} == set(KERNELS), sorted(names)
    assert len(rows) == 7 + 4
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled


def test_knn_is_an_fp32_mfma(rows):
    with open(ASM) as f:
        text = f.read()
    assert text.count("v_mfma_f32_16x16x4_f32") >= 4 * 16            # four instances, four candidate blocks x four steps each
    assert "v_mfma_f64" not in text
