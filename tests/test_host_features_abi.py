"""C-ABI surface of the feature entry points (CPU): the symbols exist with the documented signatures, the geometry of the
Gram is the documented function of the shapes, and bad arguments are rejected on the host with SEGGER_EINVAL
(SEGGER_EWORKSPACE for a short workspace) and a message -- nothing is launched."""
import ctypes as C

import pytest
import torch

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address: never dereferenced, no call below launches anything
vp = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def gram(lib, n_rows=100, n_cols=40, nnz=500, ws_bytes=None, **p):
    a = {k: FAKE for k in ("indptr", "indices", "values", "weight", "S", "s", "ws")}
    a.update(p)
    if ws_bytes is None:
        ws_bytes = max(lib.segger_features_workspace_bytes(100, 40), 0)
    return lib.segger_sparse_gram(a["indptr"], a["indices"], a["values"], a["weight"], n_rows, n_cols, nnz, a["S"], a["s"],
                                  a["ws"], ws_bytes, None)


def project(lib, n_rows=100, n_cols=40, nnz=500, k=16, out_f64=0, **p):
    a = {k_: FAKE for k_ in ("indptr", "indices", "values", "weight", "V", "offset", "out")}
    a.update(p)
    return lib.segger_sparse_project(a["indptr"], a["indices"], a["values"], a["weight"], n_rows, n_cols, nnz, a["V"],
                                     a["offset"], k, a["out"], out_f64, None)


def test_symbols_signatures_and_abi_version(lib):
    i64, i32 = C.c_int64, C.c_int32
    want = {"segger_features_gram_slabs": (i64, [i64, i64]),
            "segger_features_workspace_bytes": (i64, [i64, i64]),
            "segger_sparse_gram": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, i64, vp]),
            "segger_sparse_project": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, vp, vp, i32, vp, i32, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    import segger_amd
    from segger_amd import features
    for name in ("expression_features", "sparse_gram", "sparse_project", "cluster_cosine_similarity"):
        assert getattr(segger_amd, name) is getattr(features, name)


def test_slabs_and_workspace_are_functions_of_the_shapes(lib):
    slabs, ws = lib.segger_features_gram_slabs, lib.segger_features_workspace_bytes
    rows = _lib.FEATURES_SLAB_ROWS
    assert [slabs(n, 40) for n in (0, 1, rows - 1, rows, rows + 1, 3 * rows + 5)] == [1, 1, 1, 1, 2, 4]
    assert slabs(10 ** 6, 40) == _lib.FEATURES_MAX_SLABS
    assert slabs(10 ** 6, 500) == 29                                   # 8 tiles -> 36 pairs -> ceil(1024 / 36)
    assert slabs(10 ** 6, 4000) == 1                                   # 2016 pairs are workgroups enough
    tile = _lib.FEATURES_TILE
    for n, g in ((1, 1), (513, 65), (10 ** 6, 500), (10 ** 7, 500)):
        t = -(-g // tile)
        assert ws(n, g) == slabs(n, g) * (t * (t + 1) // 2 * tile * tile + t * tile) * 8
    assert ws(10 ** 7, 500) == ws(10 ** 6, 500) < 40 << 20             # it does not follow n_rows * n_cols
    for fn in (slabs, ws):
        assert fn(-1, 40) == EINVAL and b"negative" in lib.segger_last_error()
        assert fn(1 << 31, 40) == EINVAL and b"2^31" in lib.segger_last_error()
        assert fn(10, 0) == EINVAL and b"n_cols" in lib.segger_last_error()
        assert fn(10, _lib.FEATURES_MAX_COLS + 1) == EINVAL and b"n_cols" in lib.segger_last_error()


def test_gram_rejections(lib):
    assert gram(lib, n_rows=-1) == EINVAL and b"negative" in lib.segger_last_error()
    assert gram(lib, n_rows=1 << 31) == EINVAL and b"2^31" in lib.segger_last_error()
    assert gram(lib, n_cols=0) == EINVAL and b"n_cols" in lib.segger_last_error()
    assert gram(lib, n_cols=_lib.FEATURES_MAX_COLS + 1) == EINVAL and b"n_cols" in lib.segger_last_error()
    assert gram(lib, nnz=-1) == EINVAL and b"nnz" in lib.segger_last_error()
    assert gram(lib, ws_bytes=-1) == EINVAL and b"workspace_bytes" in lib.segger_last_error()
    for name in ("indptr", "indices", "values", "weight", "S", "s", "ws"):
        assert gram(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    for name in ("indptr", "weight", "S", "s"):
        assert gram(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in lib.segger_last_error(), name
    for name in ("indices", "values"):
        assert gram(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in lib.segger_last_error(), name
    assert gram(lib, ws=FAKE + 64) == EINVAL and b"256-byte aligned" in lib.segger_last_error()
    need = lib.segger_features_workspace_bytes(100, 40)
    assert gram(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.segger_last_error()
    assert gram(lib, n_rows=0, S=None) == EINVAL and b"NULL" in lib.segger_last_error()      # checked before the empty case


def test_project_rejections(lib):
    assert project(lib, n_rows=-1) == EINVAL and b"negative" in lib.segger_last_error()
    assert project(lib, n_cols=0) == EINVAL and b"n_cols" in lib.segger_last_error()
    assert project(lib, nnz=-1) == EINVAL and b"nnz" in lib.segger_last_error()
    for k in (0, -1, _lib.FEATURES_MAX_K + 1):
        assert project(lib, k=k) == EINVAL and b"k = " in lib.segger_last_error(), k
    assert project(lib, out_f64=2) == EINVAL and b"out_f64" in lib.segger_last_error()
    for name in ("indptr", "indices", "values", "weight", "V", "offset", "out"):
        assert project(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    for name in ("V", "offset"):
        assert project(lib, **{name: FAKE + 4}) == EINVAL and b"aligned" in lib.segger_last_error(), name
    assert project(lib, out=FAKE + 4, out_f64=1) == EINVAL and b"aligned" in lib.segger_last_error()
    assert project(lib, out=FAKE + 2) == EINVAL and b"aligned" in lib.segger_last_error()
    assert project(lib, n_rows=0, indptr=None, out=None) == 0          # no rows: nothing to do, nothing launched
    assert project(lib, n_rows=0, k=0) == EINVAL                       # the sizes are still checked


def test_python_side_rejects_cpu_tensors_and_bad_shapes():
    from segger_amd import features
    expr = {"indptr": torch.tensor([0, 1]), "indices": torch.tensor([0], dtype=torch.int32),
            "counts": torch.tensor([3], dtype=torch.int32), "gene_ids": torch.tensor([0], dtype=torch.int32)}
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        features.expression_features(expr)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        features.sparse_gram(expr["indptr"], expr["indices"], expr["counts"], torch.ones(1, dtype=torch.float64), 1)


def test_cluster_cosine_similarity_on_the_cpu():
    """plain torch, no kernel: it runs anywhere; against the reference's definition worked out by hand"""
    from segger_amd.features import cluster_cosine_similarity
    emb = torch.tensor([[3.0, 4.0], [0.0, 2.0], [5.0, 0.0], [0.0, -1.0]], dtype=torch.float64)
    labels = torch.tensor([2, -1, 2, 7])
    got = cluster_cosine_similarity(emb, labels)                       # clusters -1: (0, 1); 2: mean((.6, .8), (1, 0)); 7: (0, -1)
    means = torch.tensor([[0.0, 1.0], [0.8, 0.4], [0.0, -1.0]], dtype=torch.float64)
    assert torch.allclose(got, means @ means.T, atol=1e-15) and got.shape == (3, 3)
