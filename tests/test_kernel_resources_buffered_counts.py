"""Register audit of the buffered-counts translation unit (no GPU), from the gfx950 assembly `make asm` emits and
tools/kernel_resources.py reads: no kernel of buffered_counts.s may use scratch memory, and the static LDS of the polygon
kernels is what include/segger_amd.h states for each tier -- 4 G + 4 SEGGER_BCOUNT_TOUCHED bytes a wave, G = 2048 (four
waves on the register ring route) or SEGGER_BCOUNT_MAX_GENES, plus the 64 KB ring stage on the long-ring route, which at
the large tier is exactly the 160 KB a workgroup can use."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("bcount_keys_kernel", "bcount_cells_kernel", "bcount_bin_kernel", "bcount_short_kernel", "bcount_long_kernel",
           "counts_to_offsets_kernel")


@pytest.fixture(scope="module")
def rows():
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):                  # one translation unit: under a minute
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "../../build/asm/buffered_counts.s"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return [r for r in kernel_resources.kernels() if r["file"] == "buffered_counts.s"]


def test_buffered_counts_kernels_use_no_scratch_and_the_stated_lds(rows):
    from segger_amd import _lib

    def short(r):
        return r["name"].split("(")[0].split("<")[0].split(" ")[-1].split("::")[-1]
    own = [r for r in rows if short(r) in KERNELS]                    # the rest is rocprim's sort
    assert sorted({short(r) for r in own}) == sorted(KERNELS), sorted({short(r) for r in own})
    spilled = {r["name"][:120]: r["scratch"] for r in rows if r["scratch"]}
    assert not spilled, spilled
    ring, lst = _lib.MORPH_MAX_VERTS * 16, 4 * _lib.BCOUNT_TOUCHED
    small, large = 4 * _lib.BCOUNT_SMALL_GENES + lst, 4 * _lib.BCOUNT_MAX_GENES + lst
    lds = {}
    for r in own:
        if short(r) in ("bcount_short_kernel", "bcount_long_kernel"):
            fill, big = (w.strip() == "true" for w in r["name"].split("<")[1].split(">")[0].split(","))
            lds[(short(r), fill, big)] = r["lds"]
    assert len(lds) == 8                                             # {short, long} x {count, fill} x {small, large}
    for fill in (False, True):
        assert lds[("bcount_short_kernel", fill, False)] == 4 * small == 40960
        assert lds[("bcount_short_kernel", fill, True)] == large == 98304
        assert lds[("bcount_long_kernel", fill, False)] == ring + small == 75776
        assert lds[("bcount_long_kernel", fill, True)] == ring + large == _lib.BCOUNT_LDS_BYTES == 163840
    assert all(r["lds"] <= 128 for r in own if short(r) not in ("bcount_short_kernel", "bcount_long_kernel"))
