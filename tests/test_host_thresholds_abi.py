"""C-ABI surface of the per-gene thresholds entry points (CPU): bad arguments are rejected on the host with SEGGER_EINVAL
(SEGGER_EWORKSPACE for a short workspace) and a message, and nothing is launched.  Every call below is one that the host
checks reject: the pointers are fakes.  (An accepted ``n_rows == 0`` build fills the per-gene outputs on the device, so its
success is tested in tests/test_gpu_thresholds.py; here only its checks are.)"""
import pytest
import torch

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address: never dereferenced, no call below launches anything

POINTERS8 = ("threshold", "yen", "li", "count", "counters")
POINTERS4 = ("sim", "gene", "cell")
ROWS = POINTERS4 + ("ws",)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def build(lib, n=100, n_genes=5, max_iter=250, ws_bytes=None, **p):
    a = {k: FAKE for k in POINTERS8 + POINTERS4 + ("converged", "ws")}
    a.update(p)
    if ws_bytes is None:
        ws_bytes = max(lib.segger_thresholds_workspace_bytes(max(min(n, (1 << 31) - 1), 0), 5), 0)
    return lib.segger_thresholds_build(a["sim"], a["gene"], a["cell"], n, n_genes, max_iter, a["threshold"], a["yen"], a["li"],
                                       a["count"], a["converged"], a["counters"], a["ws"], ws_bytes, None)


def test_symbols_and_abi_version(lib):
    assert hasattr(lib, "segger_thresholds_workspace_bytes") and hasattr(lib, "segger_thresholds_build")
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    assert _lib.THRESHOLDS_CHUNK == 1024


def test_workspace_bytes(lib):
    ws = lib.segger_thresholds_workspace_bytes
    sizes = [ws(n, 5) for n in (0, 1, 1000, 1_000_000, 100_000_000)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and len(set(sizes[1:])) == 4
    for n, got in zip((1000, 1_000_000, 100_000_000), sizes[2:]):
        assert got >= 16 * n
    # 16 B per row + the sort's storage (at most one more key array, 8 B per row, and its histograms) + O(n_genes) +
    # O(n_rows / chunk): far below the torch route's 60 B per row
    assert sizes[4] < 25 * 100_000_000
    assert ws(1_000_000, 5) <= ws(1_000_000, 50_000) <= ws(1_000_000, 5) + 17 * 50_000 + 4096
    assert ws(-1, 5) == EINVAL and b"negative" in lib.segger_last_error()
    assert ws(1 << 31, 5) == EINVAL and b"2^31" in lib.segger_last_error()
    assert ws(10, 0) == EINVAL and b"n_genes" in lib.segger_last_error()
    assert ws(10, -2) == EINVAL and b"n_genes" in lib.segger_last_error()
    assert ws(10, 1 << 31) == EINVAL and b"int32" in lib.segger_last_error()
    assert ws((1 << 31) - 1, (1 << 31) - 1) > 0                        # the largest sizes: no overflow


def test_build_rejects_bad_sizes(lib):
    assert build(lib, n=-1) == EINVAL and b"negative" in lib.segger_last_error()
    assert build(lib, n=1 << 31) == EINVAL and b"2^31" in lib.segger_last_error()
    assert build(lib, n_genes=0) == EINVAL and b"n_genes" in lib.segger_last_error()
    assert build(lib, n_genes=1 << 31) == EINVAL and b"int32" in lib.segger_last_error()
    assert build(lib, max_iter=0) == EINVAL and b"max_iter" in lib.segger_last_error()
    assert build(lib, max_iter=-5) == EINVAL and b"max_iter" in lib.segger_last_error()
    assert build(lib, ws_bytes=-1) == EINVAL and b"negative workspace" in lib.segger_last_error()


def test_build_rejects_bad_pointers(lib):
    for name in POINTERS8 + POINTERS4 + ("converged", "ws"):
        assert build(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    for name in POINTERS8:
        assert build(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in lib.segger_last_error(), name
    for name in POINTERS4:
        assert build(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in lib.segger_last_error(), name
    assert build(lib, ws=FAKE + 64) == EINVAL and b"256-byte aligned" in lib.segger_last_error()


def test_short_workspace(lib):
    need = lib.segger_thresholds_workspace_bytes(100, 5)
    assert build(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.segger_last_error()
    assert build(lib, ws_bytes=0) == EWORKSPACE


def test_empty_build_still_checks_its_outputs(lib):
    """n_rows == 0 looks at no row pointer and no workspace, but the per-gene outputs it fills are checked as ever."""
    rows = {k: None for k in ROWS}
    for name in POINTERS8 + ("converged",):
        assert build(lib, n=0, ws_bytes=0, **rows, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    for name in POINTERS8:
        assert build(lib, n=0, ws_bytes=0, **rows, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in lib.segger_last_error()
    assert build(lib, n=0, n_genes=0) == EINVAL and b"n_genes" in lib.segger_last_error()
    assert build(lib, n=0, max_iter=0) == EINVAL and b"max_iter" in lib.segger_last_error()


def test_gene_thresholds_rejects_cpu_tensors():
    from segger_amd import postprocess as pp
    sim, gene, cell = torch.tensor([0.5, 0.6, 0.7]), torch.tensor([0, 0, 1]), torch.tensor([0, 1, -1])
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        pp.gene_thresholds(sim, gene, cell)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        pp.assign_transcripts_to_cells([(torch.arange(3), cell, sim, gene)], thresholds="kernel")
    import segger_amd
    assert segger_amd.gene_thresholds is pp.gene_thresholds


def test_unknown_route_is_a_value_error():
    from segger_amd import postprocess as pp
    acc = pp.SegmentationAccumulator.__new__(pp.SegmentationAccumulator)          # no device: the route is checked first
    with pytest.raises(ValueError, match="bogus"):
        acc.segmentation(thresholds="bogus")
    with pytest.raises(ValueError, match="bogus"):
        acc.expression(thresholds="bogus")
    preds = [(torch.arange(3), torch.tensor([0, 1, -1]), torch.tensor([0.5, 0.6, 0.7]), torch.tensor([0, 0, 1]))]
    with pytest.raises(ValueError, match="bogus"):
        pp.assign_transcripts_to_cells(preds, thresholds="bogus")
    assert pp.assign_transcripts_to_cells(preds, thresholds="torch")["similarity_threshold"].shape == (3,)
