"""Register audit of the fragment translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of fragments.s may use scratch memory, and the LDS of the update kernel is the
wave-private strip DESIGN 3.5p states -- 16 bytes a lane, 4096 B a workgroup, on the gather route only."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("fragments_update_kernel", "fragments_flatten_kernel", "fragments_flag_kernel", "fragments_rank_kernel",
           "fragments_label_kernel", "counts_to_offsets_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/fragments.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "fragments.s"]


def test_fragment_kernels_use_no_scratch_and_the_stated_lds(rows):
    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1]
    assert sorted({short(r) for r in rows}) == sorted(KERNELS), sorted({short(r) for r in rows})
    update = [r for r in rows if short(r) == "fragments_update_kernel"]
    assert len(update) == 3 * 2 + 2 * 2                              # three types x {pieces, elements}; two routes without rows
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    assert sorted(r["lds"] for r in update) == [0] * 4 + [4096] * 6
    assert all(r["lds"] <= 128 for r in rows if short(r) != "fragments_update_kernel")
