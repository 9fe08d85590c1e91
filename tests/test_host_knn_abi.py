"""C-ABI surface of the grid kNN entry points (CPU): bad arguments are rejected on the host with SEGGER_EINVAL and a
message, a short workspace with SEGGER_EWORKSPACE -- nothing is launched -- and an empty query set is a no-op."""
import math

import pytest

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4
FAKE = 0x1000                     # a non-NULL, aligned address: never dereferenced, every call below returns on the host


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def knn(lib, points=FAKE, n=100, queries=FAKE, m=50, k=8, max_dist=math.inf, x0=0.0, y0=0.0, cell=1.0, nx=10, ny=10, nbr=FAKE,
        dist=FAKE, ws=FAKE, ws_bytes=0):
    return lib.segger_knn_grid(points, n, queries, m, k, max_dist, x0, y0, cell, nx, ny, nbr, dist, ws, ws_bytes, None)


def test_rejects_bad_arguments(lib):
    for k in (0, 65, -3):
        assert knn(lib, k=k) == EINVAL and b"k must be in [1, 64]" in lib.segger_last_error(), k
    assert knn(lib, n=-1) == EINVAL and b"negative size" in lib.segger_last_error()
    assert knn(lib, m=-1) == EINVAL and b"negative size" in lib.segger_last_error()
    for cell in (0.0, -1.0, math.nan):
        assert knn(lib, cell=cell) == EINVAL and b"bad grid" in lib.segger_last_error(), cell
    for nx, ny in ((0, 10), (10, 0), (-1, 10), (1 << 16, 1 << 15), (46341, 46341), (2 ** 31 - 1, 1)):
        assert knn(lib, nx=nx, ny=ny) == EINVAL and b"bad grid" in lib.segger_last_error(), (nx, ny)
    for max_dist in (0.0, -2.0, math.nan, -math.inf):
        assert knn(lib, max_dist=max_dist) == EINVAL and b"max_dist must be positive" in lib.segger_last_error(), max_dist
    assert knn(lib, queries=None, m=50) == EINVAL and b"queries NULL but n_queries != n_points" in lib.segger_last_error()
    assert knn(lib, nbr=None) == EINVAL and b"nbr is NULL" in lib.segger_last_error()
    assert knn(lib, points=None) == EINVAL and b"points is NULL" in lib.segger_last_error()


def test_short_workspace(lib):
    need = lib.segger_knn_workspace_bytes(100, 10, 10)
    assert knn(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.segger_last_error()
    assert knn(lib, ws=None, ws_bytes=need) == EWORKSPACE
    assert knn(lib, queries=None, m=100, ws_bytes=0) == EWORKSPACE     # queries == NULL with matching sizes gets this far
    assert knn(lib, dist=None, ws_bytes=0) == EWORKSPACE               # so does dist == NULL


def test_no_queries_is_a_no_op(lib):
    assert knn(lib, m=0) == 0
    assert knn(lib, m=0, points=None, queries=None, nbr=None, dist=None, ws=None, n=0) == 0
    assert knn(lib, m=0, k=0) == EINVAL                                # the sizes are still checked


def test_workspace_bytes(lib):
    size = lib.segger_knn_workspace_bytes
    for n, nx, ny in ((0, 10, 10), (-5, 10, 10), (100, 0, 10), (100, 10, 0), (0, 0, 0)):
        assert size(n, nx, ny) == 256, (n, nx, ny)
    ns = (1, 2, 63, 64, 65, 1000, 4097, 100_000, 1_000_000, 20_000_000)
    by_n = [size(n, 100, 100) for n in ns]
    assert all(a <= b for a, b in zip(by_n, by_n[1:])) and by_n[0] > 256 and by_n[-1] > by_n[0]
    assert by_n[-1] >= 20_000_000 * 24                                 # four 4-byte arrays and the sorted coordinates
    grids = ((1, 1), (2, 1), (10, 10), (100, 100), (30001, 1), (1, 30001), (1000, 1000), (30001, 30001))
    by_cells = [size(5000, nx, ny) for nx, ny in sorted(grids, key=lambda g: g[0] * g[1])]
    assert all(a <= b for a, b in zip(by_cells, by_cells[1:])) and by_cells[-1] >= 30001 * 30001 * 4
    assert all(b % 256 == 0 for b in by_n + by_cells)
