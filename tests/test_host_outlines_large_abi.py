"""C-ABI surface of segger_cell_outlines_large (CPU): the two symbols exist with the documented signatures next to the
unchanged segger_cell_outlines, the ABI version is still 32, the workspace size has the documented terms, bad arguments are
rejected on the host with SEGGER_EINVAL and a message, and an empty input returns 0 without a device -- nothing is launched
by any call below (every pointer is a fake aligned address that is never dereferenced).  The Python wrapper refuses bad
``large_cells`` and ``_lds_max_points`` before anything is launched, and the canonical oracle of the large-cell tests equals
``outline_cases.outline`` wherever the triangulation is unique."""
import ctypes as C

import numpy as np
import pytest
import torch

import outline_cases as oc
import outline_large_cases as lc
from segger_amd import _lib
from test_host_outlines_abi import EINVAL, FAKE, PTRS, f64, i32, i64, vp


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, N=100, n_cells=10, connectivity=2.0, smoothing=0, capacity=100, ws_bytes=1 << 24, lds_max=2048, large_rows=0, **p):
    a = {name: FAKE for name in PTRS}
    a.update(p)
    return lib.segger_cell_outlines_large(a["xy"], a["cell"], a["keep"], N, n_cells, connectivity, smoothing, a["ring_offsets"],
                                          a["xy_out"], capacity, a["cell_ids"], a["n_transcripts"], a["counters"], a["workspace"],
                                          ws_bytes, lds_max, large_rows, None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_cell_outlines_large_workspace_bytes": (C.c_int64, [i64, i64, i64]),
            "segger_cell_outlines_large": (C.c_int, [vp, vp, vp, i64, i64, f64, i32, vp, vp, i64, vp, vp, vp, vp, i64, i32, i64, vp]),
            "segger_cell_outlines_workspace_bytes": (C.c_int64, [i64, i64]),
            "segger_cell_outlines": (C.c_int, [vp, vp, vp, i64, i64, f64, i32, vp, vp, i64, vp, vp, vp, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION                  # purely additive
    assert (_lib.OUTLINE_MAX_POINTS, _lib.OUTLINE_COUNTERS, _lib.OUTLINE_LARGE_COUNTERS) == (2048, 10, 13)
    from segger_amd import boundaries as bd
    assert len(bd.LARGE_OUTLINE_COUNTER_NAMES) == 13 and bd.LARGE_OUTLINE_COUNTER_NAMES[:10] == bd.OUTLINE_COUNTER_NAMES


def test_workspace_size_has_the_documented_terms(lib):
    def up(x):
        return (x + 255) // 256 * 256
    size = lib.segger_cell_outlines_large_workspace_bytes
    for N, n_cells in ((0, 1), (1, 1), (100, 7), (5000, 10 ** 6), (10 ** 6, 6000)):
        c = max(min(N, n_cells), 1)
        before = None
        for R in sorted({0, min(N, 1), min(N, 17), N // 2, N}):
            r = max(R, 1)
            large = up(4 * c) + up(8 * c) + up(16 * r) + up(r) + 2 * up(24 * r) + up(6 * r) + up(8 * r) + up(64 * r) + up(32 * r)
            got = size(N, n_cells, R)
            assert got == lib.segger_cell_outlines_workspace_bytes(N, n_cells) + large, (N, n_cells, R)
            assert before is None or got >= before, (N, n_cells, R)          # monotone in large_rows
            before = got
    assert size(10 ** 6, 10, 10 ** 6) - size(10 ** 6, 10, 0) <= 175 * 10 ** 6 + 8 * 256
    for N, n_cells, R in ((-1, 1, 0), ((1 << 31) - 1, 1, 0), (10, 0, 0), (10, 1 << 31, 0)):
        assert size(N, n_cells, R) == EINVAL, (N, n_cells, R)
    for R in (-1, 11):
        assert size(10, 3, R) == EINVAL and b"large_rows" in lib.segger_last_error(), R


def test_rejections(lib):
    err = lib.segger_last_error
    assert call(lib, N=-1) == EINVAL and b"negative n_rows" in err()
    assert call(lib, N=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert call(lib, n_cells=0) == EINVAL and b"n_cells" in err()
    for m in (-1, 2049):
        assert call(lib, lds_max=m) == EINVAL and b"lds_max_points" in err(), m
    for r in (-1, 101):
        assert call(lib, large_rows=r) == EINVAL and b"large_rows" in err(), r
    for s in (-1, 7):
        assert call(lib, smoothing=s) == EINVAL and b"smoothing" in err(), s
    for k in (0.0, -1.0, float("inf"), float("nan")):
        assert call(lib, connectivity=k) == EINVAL and b"connectivity" in err(), k
    assert call(lib, ws_bytes=-1) == EINVAL and b"negative" in err()
    assert call(lib, capacity=-1) == EINVAL and b"negative" in err()
    for name in PTRS:
        if name != "keep":
            assert call(lib, **{name: None}) == EINVAL and b"NULL" in err(), name
    assert call(lib, keep=None, ws_bytes=0) == EINVAL and b"workspace" in err()       # keep may be NULL: the next check fires
    for name in ("xy", "xy_out"):
        assert call(lib, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), name
    for name in ("ring_offsets", "n_transcripts", "counters"):
        assert call(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("cell", "cell_ids"):
        assert call(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in err(), name
    assert call(lib, workspace=FAKE + 64) == EINVAL and b"256-byte aligned" in err()
    for lds_max, rows in ((2048, 0), (0, 100)):
        need = lib.segger_cell_outlines_large_workspace_bytes(100, 10, rows)
        assert call(lib, ws_bytes=need - 1, lds_max=lds_max, large_rows=rows) == EINVAL and str(need).encode() in err()


def test_no_rows_return_ok_without_a_device(lib):
    assert call(lib, N=0, capacity=0, ws_bytes=0, xy=None, cell=None, keep=None, xy_out=None, cell_ids=None, n_transcripts=None,
                workspace=None) == 0
    assert call(lib, N=0, counters=None) == EINVAL
    assert call(lib, N=0, large_rows=1) == EINVAL


def test_python_side_refusals():
    from segger_amd import boundaries as bd
    xy, cell = torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5, dtype=torch.int32)
    for bad in ("Global", "lds", None, True, 0):
        with pytest.raises(ValueError, match="large_cells"):
            bd.cell_outlines(xy, cell, large_cells=bad)
    for bad in (-1, 2049, 1.0, True, "0"):
        with pytest.raises(ValueError, match="_lds_max_points"):
            bd.cell_outlines(xy, cell, large_cells="global", _lds_max_points=bad)
    with pytest.raises(ValueError, match="_lds_max_points"):                   # the default route has no such knob
        bd.cell_outlines(xy, cell, _lds_max_points=0)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        bd.cell_outlines(xy, cell, large_cells="global", _lds_max_points=0)


def test_canonical_oracle_equals_the_unique_triangulation_and_fans_the_lattice():
    for c, p in oc.scene_cells().items():
        for k in oc.CONNECTIVITIES:
            a, b = oc.outline(p, k), lc.outline_canonical(p, k)[0]
            assert (a is None and b is None) or np.array_equal(a, b), (c, k)
    big = lc.limit_cell()
    assert oc.check_case(big, 2.0)["triangles"] > 4000 and np.array_equal(oc.outline(big, 2.0), lc.check_large(big, 2.0)[0])
    g = np.stack(np.meshgrid(np.arange(9.0), np.arange(9.0)), -1).reshape(-1, 2)
    ring, area, triangles = lc.outline_canonical(np.random.default_rng(0).permutation(g), 2.0)
    assert len(ring) == 32 and area == 64.0 and triangles == 128
    assert tuple(ring[0]) == (0.0, 0.0) and tuple(ring[1]) == (1.0, 0.0)
    for name in ("repeated_cell", "many_rows_few_points"):
        assert lc.check_large(getattr(lc, name)(), 2.0)[0] is not None, name
