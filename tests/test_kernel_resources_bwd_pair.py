"""Register audit of the merged backward kernel (no GPU), by the `make asm` + tools/kernel_resources.py path of
tests/test_kernel_resources.py.  gatv2_bwd_src_dst_pair_kernel runs the tx-neighbors-tx source pass and the one-pass
tx-belongs-bd pass in one launch; all but a few thousand of its workgroups are source-pass workgroups, so it may not hold
fewer waves per SIMD than gatv2_bwd_src_kernel does by itself, and it may not touch scratch memory."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TYPES = ("float", "bf16_t", "f16_t")
VGPR_FILE, GRANULE = 512, 8                      # registers per SIMD lane, allocation granule (gfx950)


def waves_per_simd(vgpr):
    return min(8, VGPR_FILE // (-(-vgpr // GRANULE) * GRANULE))


@pytest.fixture(scope="module")
def table():
    from test_kernel_resources import _norm
    if shutil.which("make") is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    if not os.environ.get("SEGGER_SKIP_ASM_BUILD"):
        subprocess.run(["make", "-C", os.path.join(ROOT, "segger_amd", "csrc"), "asm", "-j8"], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    import kernel_resources
    return {_norm(r["name"]): r for r in kernel_resources.kernels()}


@pytest.mark.parametrize("t", TYPES)
def test_flagship_merged_kernel_has_no_scratch_and_three_waves(table, t):
    r = table[f"gatv2_bwd_src_dst_pair_kernel<{t},2,8>"]
    assert r["scratch"] == 0, r
    assert r["vgpr"] <= 168 and waves_per_simd(r["vgpr"]) >= 3, r


@pytest.mark.parametrize("t", TYPES)
def test_flagship_merged_kernel_keeps_the_source_pass_occupancy(table, t):
    """What made the merged launch lose at large batches: built for three waves it took 166-168 registers while the 16-bit
    source pass alone takes <= 128, i.e. runs four waves per SIMD."""
    pair, src = table[f"gatv2_bwd_src_dst_pair_kernel<{t},2,8>"], table[f"gatv2_bwd_src_kernel<{t},2,8,false>"]
    assert waves_per_simd(pair["vgpr"]) >= waves_per_simd(src["vgpr"]), (pair, src)


@pytest.mark.parametrize("t", ("bf16_t", "f16_t"))
@pytest.mark.parametrize("geo", ["2,8", "1,8", "3,4", "4,4"])
def test_four_wave_geometries_have_no_scratch(table, t, geo):
    """The geometries BwdPairCfg builds for four waves per SIMD: 128 registers, nothing spilled."""
    r = table[f"gatv2_bwd_src_dst_pair_kernel<{t},{geo}>"]
    assert r["scratch"] == 0 and r["vgpr"] <= 128, r


def test_slab_sum_kernels_have_no_scratch(table):
    for n in ("slab_reduce_stage1_pair", "slab_reduce_stage2_pair", "slab_reduce_stage1", "slab_reduce_stage2"):
        assert table[n]["scratch"] == 0, (n, table[n])
