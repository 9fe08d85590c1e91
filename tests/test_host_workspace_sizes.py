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
