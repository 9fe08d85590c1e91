"""C-ABI surface of the expression-matrix entry points (CPU): bad arguments are rejected on the host with SEGGER_EINVAL
(SEGGER_EWORKSPACE for a short workspace) and a message -- nothing is launched -- and an empty build is a no-op."""
import pytest
import torch

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address: never dereferenced, no call below launches anything

POINTERS8 = ("thr", "xy", "indptr", "mean", "cell_count", "centroid", "counters")
POINTERS4 = ("cell", "gene", "sim", "cell_ids", "gene_ids", "indices", "counts")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def build(lib, n=0, n_cells=10, n_genes=5, ws_bytes=None, **p):
    a = {k: FAKE for k in POINTERS8 + POINTERS4 + ("ws",)}
    a.update(p)
    if ws_bytes is None:
        ws_bytes = max(lib.segger_expression_workspace_bytes(max(min(n, (1 << 31) - 1), 0), 10, 5), 0)
    return lib.segger_expression_build(a["cell"], a["gene"], a["sim"], a["thr"], a["xy"], n, n_cells, n_genes, a["cell_ids"],
                                       a["gene_ids"], a["indptr"], a["indices"], a["counts"], a["mean"], a["cell_count"],
                                       a["centroid"], a["counters"], a["ws"], ws_bytes, None)


def test_symbols_and_abi_version(lib):
    assert hasattr(lib, "segger_expression_workspace_bytes") and hasattr(lib, "segger_expression_build")
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION


def test_workspace_bytes(lib):
    ws = lib.segger_expression_workspace_bytes
    small, big = ws(1000, 10, 5), ws(1_000_000, 10, 5)
    assert 28 * 1000 <= small < big and big >= 28 * 1_000_000
    assert ws(0, 1, 1) > 0
    assert ws(-1, 10, 5) == EINVAL and b"negative" in lib.segger_last_error()
    assert ws(1 << 31, 10, 5) == EINVAL and b"2^31" in lib.segger_last_error()
    assert ws(10, 0, 5) == EINVAL and b"n_cells" in lib.segger_last_error()
    assert ws(10, 10, 0) == EINVAL and b"n_genes" in lib.segger_last_error()
    assert ws(10, 1 << 40, 1 << 40) == EINVAL and b"overflow" in lib.segger_last_error()


def test_build_rejects_bad_sizes(lib):
    assert build(lib, n=-1) == EINVAL and b"negative" in lib.segger_last_error()
    assert build(lib, n=1 << 31) == EINVAL and b"2^31" in lib.segger_last_error()
    assert build(lib, n_cells=0) == EINVAL and b"n_cells" in lib.segger_last_error()
    assert build(lib, n_cells=-3) == EINVAL and b"n_cells" in lib.segger_last_error()
    assert build(lib, n_genes=0) == EINVAL and b"n_genes" in lib.segger_last_error()
    assert build(lib, n_cells=1 << 40, n_genes=1 << 40) == EINVAL and b"overflow" in lib.segger_last_error()
    assert build(lib, n_cells=1 << 31) == EINVAL and b"int32" in lib.segger_last_error()
    assert build(lib, n_genes=1 << 31) == EINVAL and b"int32" in lib.segger_last_error()


def test_build_rejects_bad_pointers(lib, n=100):
    for name in POINTERS8 + POINTERS4 + ("ws",):
        if name in ("xy", "centroid"):
            continue
        assert build(lib, n=n, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    assert build(lib, n=n, xy=None) == EINVAL and b"together" in lib.segger_last_error()
    assert build(lib, n=n, centroid=None) == EINVAL and b"together" in lib.segger_last_error()
    for name in POINTERS8:
        assert build(lib, n=n, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in lib.segger_last_error(), name
    for name in POINTERS4:
        assert build(lib, n=n, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in lib.segger_last_error(), name
    assert build(lib, n=n, ws=FAKE + 64) == EINVAL and b"256-byte aligned" in lib.segger_last_error()


def test_short_workspace(lib):
    need = lib.segger_expression_workspace_bytes(100, 10, 5)
    assert build(lib, n=100, ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.segger_last_error()


def test_empty_build_launches_nothing(lib):
    assert build(lib, n=0) == 0                                      # counters (and indptr[0]) stay as the caller zeroed them
    assert build(lib, n=0, xy=None, centroid=None) == 0              # without positions
    rows = {k: None for k in POINTERS4 + ("thr", "xy", "mean", "cell_count", "centroid", "ws")}
    assert build(lib, n=0, ws_bytes=0, **rows) == 0                  # the row-sized arrays of an empty slide may be NULL
    assert build(lib, n=0, counters=None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert build(lib, n=0, indptr=None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert build(lib, n=0, n_cells=0) == EINVAL                      # the sizes are still checked


def test_expression_matrix_rejects_cpu_tensors():
    from segger_amd import postprocess as pp
    res = {"row_index": torch.arange(3), "cell_encoding": torch.tensor([0, 1, -1]), "gene": torch.tensor([0, 0, 1]),
           "similarity": torch.tensor([0.5, 0.6, 0.7]), "similarity_threshold": torch.tensor([0.1, 0.1, 0.1], dtype=torch.float64)}
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        pp.expression_matrix(res)
    import segger_amd
    assert segger_amd.expression_matrix is pp.expression_matrix and segger_amd.expression_to_scipy is pp.expression_to_scipy
