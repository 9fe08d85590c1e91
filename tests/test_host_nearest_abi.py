"""C-ABI surface of the nearest-boundaries entry points (CPU): the symbols exist with the documented signatures, the
workspace size is what the header says, the ABI version is still 32, bad arguments are rejected on the host with
SEGGER_EINVAL and a message, and an empty input returns 0 without a device -- nothing is launched by any call below (every
pointer is a fake aligned address that is never dereferenced).  The Python side refuses a k outside
1 .. SEGGER_NEAREST_MAX_K, bad shapes and CPU tensors."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
PTRS = ("points", "ring_offsets", "xy", "pair_offsets", "workspace")
COMMON = [vp, i64, vp, vp, i64, i64, vp, i32, f64, f64, f64, i32, i32, vp]
SELECT_PTRS = ("pair_offsets", "pair_key", "pair_polygon", "polygon_out", "dist2_out", "inside_out", "count_out", "counters")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, fill, N=100, P=10, V=50, predicate=0, x0=0.0, y0=0.0, cell=1.0, nx=8, ny=8, ws_bytes=1 << 24, capacity=5, **p):
    a = {name: FAKE for name in PTRS + ("pair_key", "pair_polygon")}
    a["buffer"] = None
    a.update(p)
    head = (a["points"], N, a["ring_offsets"], a["xy"], P, V, a["buffer"], predicate, x0, y0, cell, nx, ny, a["pair_offsets"])
    if fill:
        return lib.segger_nearest_boundaries_fill(*head, a["pair_key"], a["pair_polygon"], capacity, a["workspace"], ws_bytes, None)
    return lib.segger_nearest_boundaries_count(*head, a["workspace"], ws_bytes, None)


def select(lib, N=100, P=10, k=3, capacity=5, **p):
    a = {name: FAKE for name in SELECT_PTRS}
    a.update(p)
    return lib.segger_nearest_boundaries_select(a["pair_offsets"], a["pair_key"], a["pair_polygon"], capacity, N, P, k, a["polygon_out"],
                                                a["dist2_out"], a["inside_out"], a["count_out"], a["counters"], None)


def test_symbols_signatures_constants_and_abi_version(lib):
    want = {"segger_nearest_boundaries_workspace_bytes": (C.c_int64, [i64, i64, i32, i32]),
            "segger_nearest_boundaries_count": (C.c_int, COMMON + [vp, i64, vp]),
            "segger_nearest_boundaries_fill": (C.c_int, COMMON + [vp, vp, i64, vp, i64, vp]),
            "segger_nearest_boundaries_select": (C.c_int, [vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    assert (_lib.NEAREST_MAX_K, _lib.NEAREST_LANE_MAX, _lib.NEAREST_COUNTERS, _lib.NEAREST_ERR_FILL) == (16, 32, 4, _lib.PJOIN_ERR_FILL)
    import segger_amd
    from segger_amd import nearest, neighbors
    assert segger_amd.nearest is nearest and len(nearest.COUNTER_NAMES) == _lib.NEAREST_COUNTERS
    assert nearest.COUNTER_NAMES == ("n_pairs", "n_kept", "n_truncated_points", "max_count")
    for name in ("nearest_boundaries", "signed_distance"):
        assert getattr(segger_amd, name) is getattr(nearest, name)
    assert segger_amd.prediction_graph_nearest is neighbors.prediction_graph_nearest


def test_header_states_the_constants():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segger_amd.h")).read()
    for name, value in (("MAX_K", _lib.NEAREST_MAX_K), ("LANE_MAX", _lib.NEAREST_LANE_MAX), ("COUNTERS", _lib.NEAREST_COUNTERS),
                        ("ERR_FILL", _lib.NEAREST_ERR_FILL)):
        assert re.search(rf"#define SEGGER_NEAREST_{name} {value}\b", header), name
    assert re.search(r"#define SEGGER_ABI_VERSION 32\b", header)


def test_workspace_size_is_what_the_header_says(lib):
    ws, join = lib.segger_nearest_boundaries_workspace_bytes, lib.segger_polygon_join_workspace_bytes

    def up(x):
        return (x + 255) // 256 * 256
    for N, nx, ny in ((0, 1, 1), (1, 1, 1), (1000, 30, 20), (10 ** 6, 700, 700), (10 ** 7, 3000, 1500)):
        for P in (0, 1, 65, 10 ** 6, (1 << 31) - 2):
            assert ws(N, P, nx, ny) == join(N, P, nx, ny) + up(4 * max(N, 1)), (N, P)
    assert ws((1 << 31) - 2, (1 << 31) - 2, 46340, 46340) > 0           # the largest sizes: no overflow
    for bad in ((-1, 1, 1, 1), (1, -1, 1, 1), ((1 << 31) - 1, 1, 1, 1), (1, (1 << 31) - 1, 1, 1)):
        assert ws(*bad) == EINVAL, bad
        assert b"points or polygons" in lib.segger_last_error() or b"negative" in lib.segger_last_error(), bad
    for bad in ((1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 65536, 65536)):
        assert ws(*bad) == EINVAL and b"bad grid" in lib.segger_last_error(), bad


@pytest.mark.parametrize("fill", [False, True])
def test_count_and_fill_rejections(lib, fill):
    err = lib.segger_last_error
    who = b"segger_nearest_boundaries_fill" if fill else b"segger_nearest_boundaries_count"
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
        assert call(lib, fill, **{name: FAKE + 2}) == EINVAL and b"aligned" in err(), name
    for name in ("ring_offsets", "pair_offsets", "buffer"):
        assert call(lib, fill, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("points", "xy"):
        assert call(lib, fill, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), name
    need = lib.segger_nearest_boundaries_workspace_bytes(100, 10, 8, 8)
    assert call(lib, fill, ws_bytes=need - 1) == EINVAL and b"workspace" in err() and str(need).encode() in err()
    assert call(lib, fill, ws_bytes=lib.segger_polygon_join_workspace_bytes(100, 10, 8, 8)) == EINVAL and str(need).encode() in err()
    assert call(lib, fill, ws_bytes=0) == EINVAL and b"workspace" in err()
    if fill:
        assert call(lib, fill, capacity=-1) == EINVAL and b"negative capacity" in err()
        for name in ("pair_key", "pair_polygon"):
            assert call(lib, fill, **{name: None}) == EINVAL and b"NULL" in err(), name
            assert call(lib, fill, **{name: FAKE + 2}) == EINVAL and b"pair_key must be 8-byte and pair_polygon 4-byte" in err(), name
        assert call(lib, fill, pair_key=FAKE + 4) == EINVAL and b"aligned" in err()


def test_select_rejections(lib):
    err = lib.segger_last_error
    assert select(lib, N=-1) == EINVAL and b"negative" in err() and b"segger_nearest_boundaries_select" in err()
    assert select(lib, P=-1) == EINVAL and b"negative" in err()
    assert select(lib, N=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert select(lib, P=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    for k in (0, -1, 17, 1 << 20):
        assert select(lib, k=k) == EINVAL and b"SEGGER_NEAREST_MAX_K = 16" in err() and str(k).encode() in err(), k
    assert select(lib, capacity=-1) == EINVAL and b"negative capacity" in err()
    for name in SELECT_PTRS:
        assert select(lib, **{name: None}) == EINVAL and b"NULL" in err(), name
    for name in ("pair_offsets", "pair_key", "dist2_out", "counters"):
        assert select(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("pair_polygon", "polygon_out", "count_out"):
        assert select(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in err(), name


@pytest.mark.parametrize("fill", [False, True])
def test_empty_inputs_return_ok_without_a_device(lib, fill):
    nothing = dict(points=None, ring_offsets=None, xy=None, pair_offsets=None, workspace=None, pair_key=None, pair_polygon=None, ws_bytes=0)
    assert call(lib, fill, P=0, V=0, **nothing) == 0
    assert call(lib, fill, N=0, **nothing) == 0
    assert call(lib, fill, N=0, P=0) == 0
    if fill:
        assert call(lib, fill, capacity=0, pair_key=None, pair_polygon=None) == 0        # no candidate: nothing to write
    assert select(lib, N=0, **{name: None for name in SELECT_PTRS}) == 0


def test_python_side_refuses_bad_arguments_and_cpu_tensors():
    from segger_amd import nearest, neighbors
    pts = torch.rand(5, 2)
    offs, xy = torch.tensor([0, 4]), torch.rand(4, 2, dtype=torch.float64)
    for bad in (0, 17, -2, 2.5, True, None):
        with pytest.raises(ValueError, match=r"k is an int in 1 \.\. SEGGER_NEAREST_MAX_K = 16"):
            nearest.nearest_boundaries(pts, offs, xy, bad)
    with pytest.raises(ValueError, match="points"):
        nearest.nearest_boundaries(torch.zeros(5, 2, dtype=torch.int64), offs, xy, 3)
    with pytest.raises(ValueError, match="predicate"):
        nearest.nearest_boundaries(pts, offs, xy, 3, predicate="within")
    with pytest.raises(ValueError, match="points_per_cell"):
        nearest.nearest_boundaries(pts, offs, xy, 3, points_per_cell=0.0)
    for bad in (-0.5, math.nan, torch.tensor([-1.0])):
        with pytest.raises(ValueError, match="buffer must be finite and >= 0"):
            nearest.nearest_boundaries(pts, offs, xy, 3, buffer=bad)
    with pytest.raises(ValueError, match="buffer is None, a float or"):
        nearest.nearest_boundaries(pts, offs, xy, 3, buffer=torch.zeros(2))
    for call_ in (lambda: nearest.nearest_boundaries(pts, offs, xy, 3), lambda: nearest.nearest_boundaries(pts[:0], offs, xy, 3),
                  lambda: neighbors.prediction_graph_nearest(pts, offs, xy), lambda: neighbors.prediction_graph_nearest(pts, offs, xy, 2, 0.5)):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
            call_()


def test_signed_distance_is_plain_torch():
    from segger_amd import nearest
    r = {"dist2": torch.tensor([[4.0, 0.25, math.inf], [0.0, 0.0, math.inf]], dtype=torch.float64),
         "inside": torch.tensor([[True, False, False], [True, False, False]])}
    assert nearest.signed_distance(r).tolist() == [[-2.0, 0.5, math.inf], [0.0, 0.0, math.inf]]
