"""Register audit of the streaming-assignment kernels (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: none of them may use scratch memory, and the arg-max must be one no-return 64-bit
vector-memory atomic, not a compare-and-swap loop."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("assign_max_kernel", "assign_write_kernel", "assign_advance_kernel", "assign_finalize_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: seconds
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/assign.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "assign.s"]


def test_assign_kernels_use_no_scratch(rows):
    by_name = {r["name"].split("(")[0]: r for r in rows}
    assert sorted(by_name) == sorted(KERNELS), sorted(by_name)
    for name, r in by_name.items():
        assert r["scratch"] == 0 and r["lds"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)                            # 8 waves per SIMD stay possible


def test_argmax_is_one_hardware_atomic(rows):
    txt = open(os.path.join(ROOT, "build", "asm", "assign.s")).read()
    assert txt.count("global_atomic_umax_x2") == 1 and "cmpswap" not in txt
