"""Workspace sizes and slab counts of the post-processing entry points (CPU: the functions run on the host and launch
nothing).  The layouts behind them are carved by one shared rule (csrc/post_common.h); callers size their buffers with
these functions and the kernels index by the same offsets, so a change of any number here is a change of the ABI's
behaviour.

The expected integers are NOT derived: they are what the library returned at the commit before the layouts moved onto the
shared carver, written down as literals.  Shapes per function: the empty or minimum size, one row, a size just below and
just above a 256-byte boundary of the smallest region, and a large one."""
import pytest

from segger_amd import _lib

RECORDED = {
    "segger_expression_workspace_bytes": [                         # (n_rows, n_cells, n_genes)
        ((0, 1, 1), 2560), ((1, 1, 1), 2560), ((63, 63, 63), 3072), ((65, 65, 65), 5376),
        ((10 ** 6, 50000, 500), 28404736)],
    "segger_thresholds_workspace_bytes": [                         # (n_rows, n_genes)
        ((0, 1), 1792), ((1, 1), 1792), ((63, 63), 2560), ((65, 65), 3840), ((10 ** 6, 500), 16016384)],
    "segger_quadtree_workspace_bytes": [                           # (n_points, depth, max_size, leaf_cap)
        ((1, 1, 1, 1), 2816), ((63, 4, 8, 63), 3328), ((65, 4, 8, 65), 5120), ((10 ** 6, 12, 2000, 4096), 8119296)],
    "segger_features_workspace_bytes": [                           # (n_rows, n_cols)
        ((0, 1), 33280), ((1, 1), 33280), ((512, 64), 33280), ((513, 65), 198656), ((10 ** 6, 500), 34328576)],
    "segger_features_gram_slabs": [
        ((0, 1), 1), ((1, 1), 1), ((512, 64), 1), ((513, 65), 2), ((10 ** 6, 500), 29)],
    "segger_knn_bruteforce_workspace_bytes": [                     # (n, d, k); the last region is not rounded up
        ((1, 1, 1), 264), ((63, 8, 5), 2776), ((65, 8, 5), 3112), ((1000, 16, 10), 484096),
        ((10 ** 6, 32, 30), 244000000)],
    "segger_knn_bruteforce_slabs": [
        ((1, 1, 1), 1), ((63, 8, 5), 1), ((65, 8, 5), 1), ((1000, 16, 10), 6), ((10 ** 6, 32, 30), 1)],
}


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_sizes_are_the_recorded_ones(name):
    fn = getattr(_lib.load(), name)
    got = [(args, fn(*args)) for args, _ in RECORDED[name]]
    assert got == RECORDED[name]


# The GATv2 backward's workspace: the destination pass's slab, the source pass's slab and the partials of their sum.  The
# kernels write one slab row per block, so these sizes are also the bound of what a backward may write.  Recorded from the
# library before the sizing moved onto the launchers' grid rule.  Per (heads, channels) -- three specialised geometries and
# a generic one -- and per n, the columns are: segger_gatv2_bwd_workspace_bytes(n), then _two_pass(n_dst, n_src, n_edges) at
# (n, n, 32 n - 1), (n, n, 32 n) -- an average source degree just below and at the wave-per-row threshold --,
# (0, n, 32 n - 1) and (17, n, 32 n).
GATV2_RECORDED = {
    (1, 32): [
        (0, 16, 16, 16, 16, 36096), (1, 35072, 36224, 36224, 33920, 37248), (15, 35840, 36992, 37376, 33920, 37632),
        (16, 35840, 36992, 37376, 33920, 37632), (17, 36096, 37248, 37760, 33920, 37760),
        (63, 38912, 40064, 41984, 33920, 39168), (64, 38912, 40064, 41984, 33920, 39168),
        (65, 39168, 40448, 42368, 34048, 39296), (32767, 2131968, 2198528, 3181568, 99328, 1085696),
        (32768, 2131968, 2198528, 3181568, 99328, 1085696), (65536, 2131968, 2264064, 4230144, 164864, 2134272),
        (262144, 2131968, 2657280, 10521600, 558080, 8425728), (1000000, 8034816, 10035840, 40035840, 2033792, 32037120)],
    (2, 64): [
        (0, 16, 16, 16, 16, 144384), (1, 140288, 144896, 144896, 135680, 148992),
        (15, 143360, 147968, 149504, 135680, 150528), (16, 143360, 147968, 149504, 135680, 150528),
        (17, 144384, 149504, 151040, 136192, 151040), (63, 155648, 161792, 167936, 137216, 156672),
        (64, 155648, 161792, 167936, 137216, 156672), (65, 156672, 163328, 169472, 137728, 157184),
        (32767, 8527872, 9580544, 12726272, 1183744, 4342784), (32768, 8527872, 9580544, 12726272, 1183744, 4342784),
        (65536, 8527872, 10629120, 16920576, 2232320, 8537088), (262144, 8527872, 16920576, 42086400, 8523776, 33702912),
        (1000000, 32139264, 64143360, 160143360, 32135168, 128148480)],
    (4, 64): [
        (0, 16, 16, 16, 16, 288768), (1, 280576, 289792, 289792, 271360, 297984),
        (15, 286720, 296960, 299008, 272384, 301056), (16, 286720, 296960, 299008, 272384, 301056),
        (17, 288768, 300032, 302080, 273408, 302080), (63, 311296, 327680, 335872, 278528, 313344),
        (64, 311296, 327680, 335872, 278528, 313344), (65, 313344, 330752, 338944, 279552, 314368),
        (32767, 17055744, 21258240, 25452544, 4464640, 8685568), (32768, 17055744, 21258240, 25452544, 4464640, 8685568),
        (65536, 17055744, 25452544, 33841152, 8658944, 17074176),
        (262144, 17055744, 50618368, 84172800, 33824768, 67405824),
        (1000000, 64278528, 192286720, 320286720, 128270336, 256296960)],
    (5, 24): [
        (0, 16, 16, 16, 16, 135360), (1, 131520, 131520, 131520, 122880, 135360),
        (15, 134400, 134400, 134400, 122880, 135360), (16, 134400, 134400, 134400, 122880, 135360),
        (17, 135360, 135360, 135360, 122880, 135360), (63, 145920, 145920, 145920, 122880, 135360),
        (64, 145920, 145920, 145920, 122880, 135360), (65, 146880, 146880, 146880, 122880, 135360),
        (32767, 7994880, 7994880, 7994880, 122880, 135360), (32768, 7994880, 7994880, 7994880, 122880, 135360),
        (65536, 7994880, 7994880, 7994880, 122880, 135360), (262144, 7994880, 7994880, 7994880, 122880, 135360),
        (1000000, 30130560, 30130560, 30130560, 122880, 135360)],
}


@pytest.mark.parametrize("geometry", sorted(GATV2_RECORDED))
def test_gatv2_bwd_workspace_sizes_are_the_recorded_ones(geometry):
    lib, (h, c) = _lib.load(), geometry
    one, two = lib.segger_gatv2_bwd_workspace_bytes, lib.segger_gatv2_bwd_workspace_bytes_two_pass
    got = [(n, one(n, h, c), two(n, n, 32 * n - 1, h, c), two(n, n, 32 * n, h, c), two(0, n, 32 * n - 1, h, c),
            two(17, n, 32 * n, h, c)) for n, *_ in GATV2_RECORDED[geometry]]
    assert got == GATV2_RECORDED[geometry]
    # nothing to do, or no geometry: the 16-byte minimum
    assert [two(0, 0, 0, h, c), two(-1, -5, 3, h, c), two(0, -1, 0, h, c), one(0, h, c), one(-1, h, c)] == [16] * 5
    assert [two(5, 5, 5, 0, c), two(5, 5, 5, h, 0), two(5, 5, 5, -1, c), one(5, 0, c), one(5, h, -2)] == [16] * 5
