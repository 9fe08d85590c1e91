"""C-ABI surface of the buffered-counts entry points (CPU): the symbols exist with the documented signatures, the
workspace size is what the header says, the ABI version is still 32, bad arguments are rejected on the host with
SEGGER_EINVAL and a message, and an empty input returns 0 without a device -- nothing is launched by any call below (every
pointer is a fake aligned address that is never dereferenced).  The Python side refuses bad shapes and dtypes, a panel
above SEGGER_BCOUNT_MAX_GENES (naming the cap) and CPU tensors."""
import ctypes as C
import math

import pytest
import torch

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
PTRS = ("points", "gene", "ring_offsets", "xy", "indptr", "cell_count", "workspace")
COMMON = [vp, i64, vp, i64, vp, vp, i64, i64, vp, i32, f64, f64, f64, i32, i32, vp]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, fill, N=100, G=500, P=10, V=50, predicate=0, x0=0.0, y0=0.0, cell=1.0, nx=8, ny=8, ws_bytes=1 << 24, capacity=5, **p):
    a = {name: FAKE for name in PTRS + ("counters", "indices", "counts")}
    a["buffer"] = None
    a.update(p)
    head = (a["points"], N, a["gene"], G, a["ring_offsets"], a["xy"], P, V, a["buffer"], predicate, x0, y0, cell, nx, ny, a["indptr"])
    if fill:
        return lib.segger_buffered_counts_fill(*head, a["cell_count"], a["indices"], a["counts"], capacity, a["workspace"], ws_bytes, None)
    return lib.segger_buffered_counts_count(*head, a["cell_count"], a["counters"], a["workspace"], ws_bytes, None)


def test_symbols_signatures_constants_and_abi_version(lib):
    want = {"segger_buffered_counts_workspace_bytes": (C.c_int64, [i64, i64, i64, i32, i32]),
            "segger_buffered_counts_count": (C.c_int, COMMON + [vp, vp, vp, i64, vp]),
            "segger_buffered_counts_fill": (C.c_int, COMMON + [vp, vp, vp, i64, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    # the cap: the 160 KB of LDS a workgroup can use, minus the 64 KB ring stage, minus the touched list, in int32 entries
    assert _lib.BCOUNT_LDS_BYTES == 160 * 1024 and _lib.MORPH_MAX_VERTS * 16 == 65536
    assert _lib.BCOUNT_MAX_GENES == (160 * 1024 - 65536 - 4 * _lib.BCOUNT_TOUCHED) // 4 == 24064
    assert (_lib.BCOUNT_SMALL_GENES, _lib.BCOUNT_TOUCHED, _lib.BCOUNT_COUNTERS, _lib.BCOUNT_ERR_FILL) == (2048, 512, 5, _lib.PJOIN_ERR_FILL)
    import segger_amd
    from segger_amd import buffered_counts as bcm
    assert segger_amd.buffered_counts is bcm and len(bcm.COUNTER_NAMES) == _lib.BCOUNT_COUNTERS
    assert bcm.COUNTER_NAMES == ("n_pairs", "nnz", "n_bad", "n_overflow_rows", "n_large_tier")
    for name in ("buffered_counts_regions", "buffered_counts_to_scipy", "filter_boundaries"):
        assert getattr(segger_amd, name) is getattr(bcm, name)


def test_header_states_the_constants():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segger_amd.h")).read()
    for name, value in (("SMALL_GENES", _lib.BCOUNT_SMALL_GENES), ("TOUCHED", _lib.BCOUNT_TOUCHED), ("LDS_BYTES", _lib.BCOUNT_LDS_BYTES),
                        ("COUNTERS", _lib.BCOUNT_COUNTERS), ("ERR_FILL", _lib.BCOUNT_ERR_FILL)):
        assert re.search(rf"#define SEGGER_BCOUNT_{name} {value}\b", header), name
    assert "#define SEGGER_BCOUNT_MAX_GENES ((SEGGER_BCOUNT_LDS_BYTES - 65536 - 4 * SEGGER_BCOUNT_TOUCHED) / 4)" in header


def test_workspace_size_is_what_the_header_says(lib):
    ws, join = lib.segger_buffered_counts_workspace_bytes, lib.segger_polygon_join_workspace_bytes

    def up(x):
        return (x + 255) // 256 * 256
    for N, nx, ny in ((0, 1, 1), (1, 1, 1), (1000, 30, 20), (10 ** 6, 700, 700), (10 ** 7, 3000, 1500)):
        for P in (0, 1, 65, 10 ** 6, (1 << 31) - 2):
            for G in (1, 2048, 2049, _lib.BCOUNT_MAX_GENES):
                assert ws(N, P, G, nx, ny) == join(N, P, nx, ny) + up(4 * max(N, 1)), (N, P, G)
    assert ws((1 << 31) - 2, (1 << 31) - 2, 500, 46340, 46340) > 0      # the largest sizes: no overflow
    for bad in ((-1, 1, 5, 1, 1), (1, -1, 5, 1, 1), ((1 << 31) - 1, 1, 5, 1, 1), (1, (1 << 31) - 1, 5, 1, 1)):
        assert ws(*bad) == EINVAL, bad
        assert b"points or polygons" in lib.segger_last_error() or b"negative" in lib.segger_last_error(), bad
    for G in (0, -1, _lib.BCOUNT_MAX_GENES + 1):
        assert ws(1, 1, G, 1, 1) == EINVAL and b"SEGGER_BCOUNT_MAX_GENES = 24064" in lib.segger_last_error(), G
    for bad in ((1, 1, 5, 0, 1), (1, 1, 5, 1, 0), (1, 1, 5, 65536, 65536)):
        assert ws(*bad) == EINVAL and b"bad grid" in lib.segger_last_error(), bad


@pytest.mark.parametrize("fill", [False, True])
def test_rejections(lib, fill):
    err = lib.segger_last_error
    who = b"segger_buffered_counts_fill" if fill else b"segger_buffered_counts_count"
    assert call(lib, fill, N=-1) == EINVAL and b"negative" in err() and who in err()
    assert call(lib, fill, P=-1) == EINVAL and b"negative" in err()
    assert call(lib, fill, V=-1) == EINVAL and b"negative n_vertices" in err()
    assert call(lib, fill, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
    assert call(lib, fill, N=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert call(lib, fill, P=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    for G in (0, -5, _lib.BCOUNT_MAX_GENES + 1):
        assert call(lib, fill, G=G) == EINVAL and b"n_genes" in err() and b"24064" in err(), G
    assert call(lib, fill, predicate=2) == EINVAL and b"predicate 2" in err()
    for grid in (dict(nx=0), dict(ny=-3), dict(nx=65536, ny=65536), dict(cell=0.0), dict(cell=-1.0), dict(cell=math.inf),
                 dict(cell=math.nan), dict(x0=math.nan), dict(y0=math.inf)):
        assert call(lib, fill, **grid) == EINVAL and b"bad grid" in err(), grid
    for name in PTRS:
        assert call(lib, fill, **{name: None}) == EINVAL and b"NULL" in err(), name
        assert call(lib, fill, **{name: FAKE + 2}) == EINVAL and b"aligned" in err(), name
    for name in ("ring_offsets", "indptr", "cell_count", "buffer"):
        assert call(lib, fill, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("points", "xy"):
        assert call(lib, fill, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), name
    need = lib.segger_buffered_counts_workspace_bytes(100, 10, 500, 8, 8)
    assert call(lib, fill, ws_bytes=need - 1) == EINVAL and b"workspace" in err() and str(need).encode() in err()
    assert call(lib, fill, ws_bytes=0) == EINVAL and b"workspace" in err()
    if fill:
        assert call(lib, fill, capacity=-1) == EINVAL and b"negative capacity" in err()
        for name in ("indices", "counts"):
            assert call(lib, fill, **{name: None}) == EINVAL and b"NULL" in err(), name
            assert call(lib, fill, **{name: FAKE + 2}) == EINVAL and b"indices and counts" in err(), name
    else:
        assert call(lib, fill, counters=None) == EINVAL and b"NULL" in err()
        assert call(lib, fill, counters=FAKE + 4) == EINVAL and b"cell_count and counters" in err()


@pytest.mark.parametrize("fill", [False, True])
def test_empty_inputs_return_ok_without_a_device(lib, fill):
    nothing = dict(points=None, gene=None, ring_offsets=None, xy=None, indptr=None, cell_count=None, counters=None, workspace=None,
                   indices=None, counts=None, ws_bytes=0)
    assert call(lib, fill, P=0, V=0, **nothing) == 0
    assert call(lib, fill, N=0, **nothing) == 0
    assert call(lib, fill, N=0, P=0) == 0
    if fill:
        assert call(lib, fill, capacity=0, indices=None, counts=None) == 0      # an empty matrix: nothing to write


def test_python_side_refuses_bad_arguments_the_cap_and_cpu_tensors():
    from segger_amd import buffered_counts as bcm
    cap = _lib.BCOUNT_MAX_GENES
    pts, gene = torch.rand(5, 2), torch.zeros(5, dtype=torch.int64)
    offs, xy = torch.tensor([0, 4]), torch.rand(4, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match=rf"n_genes = {cap + 1} is above SEGGER_BCOUNT_MAX_GENES = {cap}"):
        bcm.buffered_counts(pts, gene, offs, xy, cap + 1)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="n_genes is a positive int"):
            bcm.buffered_counts(pts, gene, offs, xy, bad)
    for bad in (torch.zeros(5), torch.zeros(4, dtype=torch.int64), torch.zeros(5, 1, dtype=torch.int32), torch.zeros(5, dtype=torch.bool), [0] * 5):
        with pytest.raises(ValueError, match="gene is an integer"):
            bcm.buffered_counts(pts, bad, offs, xy, 10)
    with pytest.raises(ValueError, match="points"):
        bcm.buffered_counts(torch.zeros(5, 2, dtype=torch.int64), gene, offs, xy, 10)
    with pytest.raises(ValueError, match="predicate"):
        bcm.buffered_counts(pts, gene, offs, xy, 10, predicate="within")
    with pytest.raises(ValueError, match="points_per_cell"):
        bcm.buffered_counts(pts, gene, offs, xy, 10, points_per_cell=0.0)
    for bad in (-0.5, math.nan, torch.tensor([-1.0])):
        with pytest.raises(ValueError, match="buffer must be finite and >= 0"):
            bcm.buffered_counts(pts, gene, offs, xy, 10, buffer=bad)
    with pytest.raises(ValueError, match="buffer is None, a float or"):
        bcm.buffered_counts(pts, gene, offs, xy, 10, buffer=torch.zeros(2))
    with pytest.raises(ValueError, match="four finite numbers"):
        bcm.filter_boundaries(offs, xy, (0.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0))
    for call_ in (lambda: bcm.buffered_counts(pts, gene, offs, xy, 10), lambda: bcm.buffered_counts(pts[:0], gene[:0], offs, xy, 10),
                  lambda: bcm.filter_boundaries(offs, xy, (0.0, 0.0, 1.0, 1.0), (-1.0, -1.0, 2.0, 2.0)),
                  lambda: bcm.buffered_counts_regions(pts, gene, offs, xy, 10, [[0.0, 0.0, 1.0, 1.0]], 0.5)):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
            call_()


def test_gene_codes_do_not_wrap_in_a_narrow_dtype():
    """the mapping to the kernel's int32 is plain torch and runs anywhere: n_genes and -1 must not wrap in gene's dtype"""
    from segger_amd.buffered_counts import _gene_codes
    for dtype, values in ((torch.int8, [0, 5, 100, 127, -1, -128]), (torch.uint8, [0, 5, 100, 244, 255]),
                          (torch.int16, [0, 300, -7, 32767]), (torch.int32, [0, 24063, 24064, -1]), (torch.int64, [0, 2 ** 40, -2 ** 33, 7])):
        g = torch.tensor(values, dtype=dtype)
        for n_genes in (1, 100, 128, 256, 500, 24064):
            got = _gene_codes(g, n_genes)
            assert got.dtype == torch.int32 and got.tolist() == [v if 0 <= v < n_genes else -1 for v in values], (dtype, n_genes)
