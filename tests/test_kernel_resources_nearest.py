"""Register audit of the nearest-boundaries translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of nearest_boundaries.s may use scratch memory, and the static LDS is what
include/segger_amd.h states -- the 64 KB ring stage of the long-ring route, the wave totals of the one-workgroup scan, and
nothing in any other kernel: the selection keeps no list, in registers or in LDS."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("near_keys_kernel", "near_cells_kernel", "near_bin_kernel", "near_short_kernel", "near_long_kernel", "near_select_kernel",
           "counts_to_offsets_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/nearest_boundaries.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "nearest_boundaries.s"]


def test_nearest_kernels_use_no_scratch_and_the_stated_lds(rows):
    from segger_amd import _lib

    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1]
    own = [r for r in rows if short(r) in KERNELS]                    # the rest is rocprim's sort
    assert sorted({short(r) for r in own}) == sorted(KERNELS), sorted({short(r) for r in own})
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    lds = {}
    for r in own:
        lds.setdefault(short(r), []).append(r["lds"])
    assert lds["near_long_kernel"] == [_lib.MORPH_MAX_VERTS * 16] * 2 == [65536, 65536]          # count and fill
    assert lds["near_short_kernel"] == [0, 0] and lds["near_select_kernel"] == [0]
    assert lds["counts_to_offsets_kernel"] == [128]                   # 16 wave totals of 8 bytes
    assert all(lds[name] == [0] for name in ("near_keys_kernel", "near_cells_kernel", "near_bin_kernel"))
