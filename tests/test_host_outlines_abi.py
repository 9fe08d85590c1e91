"""C-ABI surface of the concave outline entry points (CPU): the symbols exist with the documented signatures, the ABI
version is still 32, bad arguments are rejected on the host with SEGGER_EINVAL and a message, and an empty input returns 0
without a device -- nothing is launched by any call below (every pointer is a fake aligned address that is never
dereferenced).  The Python wrappers refuse bad shapes, options and CPU tensors before anything is launched, and
``cell_boundaries(method="delaunay")`` still refuses: the outlines are entry points of their own."""
import ctypes as C

import pytest
import torch

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
PTRS = ("xy", "cell", "keep", "ring_offsets", "xy_out", "cell_ids", "n_transcripts", "counters", "workspace")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, N=100, n_cells=10, connectivity=2.0, smoothing=0, capacity=100, ws_bytes=1 << 24, **p):
    a = {name: FAKE for name in PTRS}
    a.update(p)
    return lib.segger_cell_outlines(a["xy"], a["cell"], a["keep"], N, n_cells, connectivity, smoothing, a["ring_offsets"], a["xy_out"],
                                    capacity, a["cell_ids"], a["n_transcripts"], a["counters"], a["workspace"], ws_bytes, None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_cell_outlines_workspace_bytes": (C.c_int64, [i64, i64]),
            "segger_cell_outlines": (C.c_int, [vp, vp, vp, i64, i64, f64, i32, vp, vp, i64, vp, vp, vp, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION                  # purely additive
    assert (_lib.OUTLINE_MAX_POINTS, _lib.OUTLINE_COUNTERS) == (2048, 10) and _lib.OUTLINE_MAX_POINTS >= 2048
    import segger_amd
    from segger_amd import boundaries, postprocess
    for name in ("cell_outlines", "segmentation_outlines"):
        assert getattr(segger_amd, name) is getattr(boundaries, name)
    assert callable(postprocess.SegmentationAccumulator.outlines)


def test_workspace_size_has_the_documented_terms(lib):
    def up(x):
        return (x + 255) // 256 * 256
    for N, n_cells in ((0, 1), (1, 1), (100, 7), (5000, 10 ** 6), (10 ** 6, 6000)):
        n, c = max(N, 1), max(min(N, n_cells), 1)
        fixed = 256 + 2 * up(4 * c) + up(8 * n) + up(16 * n) + 4 * up(4 * c)
        got = lib.segger_cell_outlines_workspace_bytes(N, n_cells)
        assert got > fixed and (got - fixed) % 256 == 0, (N, n_cells)          # the rest is the sort's and the compaction's
    for N, n_cells in ((-1, 1), ((1 << 31) - 1, 1), (10, 0), (10, 1 << 31)):
        assert lib.segger_cell_outlines_workspace_bytes(N, n_cells) == EINVAL, (N, n_cells)
    assert b"n_cells" in lib.segger_last_error()


def test_rejections(lib):
    err = lib.segger_last_error
    assert call(lib, N=-1) == EINVAL and b"negative n_rows" in err()
    assert call(lib, N=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert call(lib, n_cells=0) == EINVAL and b"n_cells" in err()
    assert call(lib, n_cells=1 << 31) == EINVAL and b"n_cells" in err()
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
    assert call(lib, xy_out=None, capacity=0, ws_bytes=0) == EINVAL and b"workspace" in err()
    for name in ("xy", "xy_out"):
        assert call(lib, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), name
    for name in ("ring_offsets", "n_transcripts", "counters"):
        assert call(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("cell", "cell_ids"):
        assert call(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in err(), name
    assert call(lib, workspace=FAKE + 64) == EINVAL and b"256-byte aligned" in err()
    need = lib.segger_cell_outlines_workspace_bytes(100, 10)
    assert call(lib, ws_bytes=need - 1) == EINVAL and b"workspace" in err() and str(need).encode() in err()


def test_no_rows_return_ok_without_a_device(lib):
    assert call(lib, N=0, capacity=0, ws_bytes=0, xy=None, cell=None, keep=None, xy_out=None, cell_ids=None, n_transcripts=None,
                workspace=None) == 0
    assert call(lib, N=0, counters=None) == EINVAL


def test_python_side_refusals(monkeypatch):
    from segger_amd import boundaries as bd
    xy, cell = torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match=r"delaunay.*boundary\.py:57-154"):
        bd.cell_boundaries(xy, cell, method="delaunay")                        # the spelling is not routed here
    with pytest.raises(TypeError):
        bd.cell_outlines(xy, cell, method="delaunay")
    for s in (-1, 7, 1.0, True):
        with pytest.raises(ValueError, match="smoothing"):
            bd.cell_outlines(xy, cell, smoothing=s)
    for k in (0, -2.0, float("inf"), float("nan"), "2", True, None):
        with pytest.raises(ValueError, match="connectivity"):
            bd.cell_outlines(xy, cell, connectivity=k)
    for bad in (torch.zeros(5, 3), torch.zeros(10), torch.zeros(5, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="xy"):
            bd.cell_outlines(bad, cell)
    for bad in (torch.zeros(5), torch.zeros(5, 1, dtype=torch.int32), torch.zeros(5, dtype=torch.bool)):
        with pytest.raises(ValueError, match="cell"):
            bd.cell_outlines(xy, bad)
    with pytest.raises(ValueError, match="different numbers of rows"):
        bd.cell_outlines(xy, cell[:4])
    with pytest.raises(ValueError, match="different numbers of rows"):
        bd.cell_outlines(xy, cell, keep=torch.ones(4, dtype=torch.bool))
    for n_cells in (0, 1 << 31):
        with pytest.raises(ValueError, match="n_cells"):
            bd.cell_outlines(xy, cell, n_cells)
    monkeypatch.setattr(bd, "MAX_ROWS", 4)                           # stands for 2^31 - 2: no tensor of that size is made
    with pytest.raises(ValueError, match=r"2\^31"):
        bd.cell_outlines(xy, cell)
    monkeypatch.undo()
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        bd.cell_outlines(xy, cell)
    res = {"row_index": torch.arange(5), "cell_encoding": cell.long(), "similarity": torch.ones(5),
           "similarity_threshold": torch.zeros(5, dtype=torch.float64)}
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        bd.segmentation_outlines(res, xy)
