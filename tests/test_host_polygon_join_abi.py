"""C-ABI surface of the polygon join entry points (CPU): the symbols exist with the documented signatures, the workspace
size is what the header says, the ABI version is still 32, bad arguments are rejected on the host with SEGGER_EINVAL and
a message, and an empty input returns 0 without a device -- nothing is launched by any call below (every pointer is a
fake aligned address that is never dereferenced).  The Python side refuses bad shapes and dtypes, a negative buffer, a
ring above SEGGER_MORPH_MAX_VERTS and CPU tensors."""
import ctypes as C
import math

import pytest
import torch

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
PTRS = ("points", "ring_offsets", "xy", "pair_offsets", "workspace")
COMMON = [vp, i64, vp, vp, i64, i64, vp, i32, f64, f64, f64, i32, i32, vp]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, fill, N=100, P=10, V=50, predicate=0, x0=0.0, y0=0.0, cell=1.0, nx=8, ny=8, ws_bytes=1 << 24, capacity=5, **p):
    a = {name: FAKE for name in PTRS + ("out",)}
    a["buffer"] = None
    a.update(p)
    head = (a["points"], N, a["ring_offsets"], a["xy"], P, V, a["buffer"], predicate, x0, y0, cell, nx, ny, a["pair_offsets"])
    if fill:
        return lib.segger_polygon_join_fill(*head, a["out"], capacity, a["workspace"], ws_bytes, None)
    return lib.segger_polygon_join_count(*head, a["workspace"], ws_bytes, None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_polygon_join_workspace_bytes": (C.c_int64, [i64, i64, i32, i32]),
            "segger_polygon_join_count": (C.c_int, COMMON + [vp, i64, vp]),
            "segger_polygon_join_fill": (C.c_int, COMMON + [vp, i64, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    assert (_lib.PJOIN_CONTAINS, _lib.PJOIN_INTERSECTS) == (0, 1)
    assert (_lib.PJOIN_ERR_OFFSETS, _lib.PJOIN_ERR_CAP, _lib.PJOIN_ERR_BUFFER, _lib.PJOIN_ERR_FILL) == (1, 2, 4, 8)
    import segger_amd
    from segger_amd import geometry, neighbors
    assert segger_amd.geometry is geometry
    assert segger_amd.points_in_polygons is geometry.points_in_polygons
    assert segger_amd.prediction_graph_shape is neighbors.prediction_graph_shape


def test_workspace_size_is_what_the_header_says(lib):
    ws = lib.segger_polygon_join_workspace_bytes

    def up(x):
        return (x + 255) // 256 * 256

    def fixed(N, P, nx, ny):
        n = max(N, 1)
        return 256 + up(8 * n) + up(16 * n) + up(4 * (nx * ny + 1)) + 2 * up(4 * P)
    for N, nx, ny in ((0, 1, 1), (1, 1, 1), (1000, 30, 20), (10 ** 6, 700, 700), (10 ** 7, 3000, 1500)):
        sort = ws(N, 0, nx, ny) - fixed(N, 0, nx, ny)                 # the sort's storage: depends on N and nx ny only
        assert 0 < sort <= up(8 * max(N, 1)) + (1 << 20), (N, sort)   # at most one more key array and its histograms
        for P in (1, 63, 64, 65, 1000, 10 ** 6, (1 << 31) - 2):
            assert ws(N, P, nx, ny) == fixed(N, P, nx, ny) + sort, (N, P)
    assert ws((1 << 31) - 2, (1 << 31) - 2, 46340, 46340) > 0          # the largest sizes: no overflow
    for bad in ((-1, 1, 1, 1), (1, -1, 1, 1), ((1 << 31) - 1, 1, 1, 1), (1, (1 << 31) - 1, 1, 1)):
        assert ws(*bad) == EINVAL, bad
        assert b"points or polygons" in lib.segger_last_error() or b"negative" in lib.segger_last_error(), bad
    for bad in ((1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 65536, 65536)):
        assert ws(*bad) == EINVAL and b"bad grid" in lib.segger_last_error(), bad


@pytest.mark.parametrize("fill", [False, True])
def test_rejections(lib, fill):
    err = lib.segger_last_error
    who = b"segger_polygon_join_fill" if fill else b"segger_polygon_join_count"
    assert call(lib, fill, N=-1) == EINVAL and b"negative" in err() and who in err()
    assert call(lib, fill, P=-1) == EINVAL and b"negative" in err()
    assert call(lib, fill, V=-1) == EINVAL and b"negative n_vertices" in err()
    assert call(lib, fill, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
    assert call(lib, fill, N=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert call(lib, fill, P=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert call(lib, fill, predicate=2) == EINVAL and b"predicate 2" in err()
    for grid in (dict(nx=0), dict(ny=-3), dict(nx=65536, ny=65536), dict(cell=0.0), dict(cell=-1.0), dict(cell=math.inf),
                 dict(cell=math.nan), dict(x0=math.nan), dict(y0=math.inf)):
        assert call(lib, fill, **grid) == EINVAL and b"bad grid" in err(), grid
    for name in PTRS:
        assert call(lib, fill, **{name: None}) == EINVAL and b"NULL" in err(), name
        assert call(lib, fill, **{name: FAKE + 4}) == EINVAL and b"aligned" in err(), name
    assert call(lib, fill, buffer=FAKE + 4) == EINVAL and b"8-byte aligned" in err()
    for name in ("points", "xy"):
        assert call(lib, fill, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), name
    need = lib.segger_polygon_join_workspace_bytes(100, 10, 8, 8)
    assert call(lib, fill, ws_bytes=need - 1) == EINVAL and b"workspace" in err() and str(need).encode() in err()
    assert call(lib, fill, ws_bytes=0) == EINVAL and b"workspace" in err()
    if fill:
        assert call(lib, fill, capacity=-1) == EINVAL and b"negative capacity" in err()
        assert call(lib, fill, out=None) == EINVAL and b"NULL" in err()
        assert call(lib, fill, out=FAKE + 4) == EINVAL and b"point_index_out" in err()


@pytest.mark.parametrize("fill", [False, True])
def test_empty_inputs_return_ok_without_a_device(lib, fill):
    nothing = dict(points=None, ring_offsets=None, xy=None, pair_offsets=None, workspace=None, out=None, ws_bytes=0)
    assert call(lib, fill, P=0, V=0, **nothing) == 0
    assert call(lib, fill, N=0, **nothing) == 0
    assert call(lib, fill, N=0, P=0) == 0
    if fill:
        assert call(lib, fill, capacity=0, out=None) == 0               # no pairs: nothing to write, nothing launched


def test_python_side_refuses_bad_arguments_the_cap_and_cpu_tensors():
    from segger_amd import geometry as ge, neighbors as nb
    cap = _lib.MORPH_MAX_VERTS
    pts = torch.rand(5, 2)
    offs, xy = torch.tensor([0, 4]), torch.rand(4, 2, dtype=torch.float64)
    for bad in (torch.rand(5, 3), torch.rand(10), torch.zeros(5, 2, dtype=torch.int64), [[0.0, 0.0]]):
        with pytest.raises(ValueError, match="points"):
            ge.points_in_polygons(bad, offs, xy)
    with pytest.raises(ValueError, match="ring_offsets"):
        ge.points_in_polygons(pts, torch.zeros(3, dtype=torch.float32), xy)
    with pytest.raises(ValueError, match="xy"):
        ge.points_in_polygons(pts, offs, torch.zeros(4, 3))
    with pytest.raises(ValueError, match="predicate"):
        ge.points_in_polygons(pts, offs, xy, predicate="within")
    with pytest.raises(ValueError, match="points_per_cell"):
        ge.points_in_polygons(pts, offs, xy, points_per_cell=0.0)
    for bad in (-0.5, math.nan, math.inf, torch.tensor([-1.0]), torch.tensor([math.nan])):
        with pytest.raises(ValueError, match="buffer must be finite and >= 0"):
            ge.points_in_polygons(pts, offs, xy, buffer=bad)
    for bad in (torch.zeros(2), torch.zeros(1, 1), torch.zeros(1, dtype=torch.int64)):
        with pytest.raises(ValueError, match="buffer is None, a float or"):
            ge.points_in_polygons(pts, offs, xy, buffer=bad)
    ring = torch.rand(cap + 1, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match=rf"polygon 1 has {cap + 1} vertices.*SEGGER_MORPH_MAX_VERTS = {cap}"):
        ge.points_in_polygons(pts, torch.tensor([0, 3, 3 + cap + 1]), torch.cat([torch.rand(3, 2, dtype=torch.float64), ring]))
    with pytest.raises(ValueError, match=rf"polygon 1 has {cap + 1} vertices"):
        nb.prediction_graph_shape(pts, torch.tensor([0, 3, 3 + cap + 1]), torch.cat([torch.rand(3, 2, dtype=torch.float64), ring]))
    for call_ in (lambda: ge.points_in_polygons(pts, offs, xy), lambda: ge.points_in_polygons(pts, offs, xy, buffer=0.25),
                  lambda: ge.points_in_polygons(pts[:0], offs, xy), lambda: nb.prediction_graph_shape(pts, offs, xy)):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
            call_()
    for bad in (-0.01, math.nan):
        with pytest.raises(ValueError, match="buffer_ratio"):
            nb.prediction_graph_shape(pts, offs, xy, buffer_ratio=bad)
