"""C-ABI surface of the phenograph entry points (CPU): the symbols exist with the documented signatures, the slab count
and workspace of the brute-force kNN are the documented functions of the shapes, and bad arguments are rejected on the
host with SEGGER_EINVAL (SEGGER_EWORKSPACE for a short workspace) and a message -- nothing is launched."""
import ctypes as C

import pytest
import torch

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address: never dereferenced, no call below launches anything
vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def knn(lib, n=100, d=8, k=5, ws_bytes=None, **p):
    a = {name: FAKE for name in ("X", "idx", "dist2", "ws")}
    a.update(p)
    if ws_bytes is None:
        ws_bytes = max(lib.segger_knn_bruteforce_workspace_bytes(100, 8, 5), 0)
    return lib.segger_knn_bruteforce(a["X"], n, d, k, a["idx"], a["dist2"], a["ws"], ws_bytes, None)


def move(lib, n=10, nnz=20, sub=0, n_sub=4, gamma=1.0, two_m=8.0, **p):
    a = {name: FAKE for name in ("indptr", "indices", "weight", "kdeg", "comm", "tot", "size", "proposal")}
    a.update(p)
    return lib.segger_louvain_move(a["indptr"], a["indices"], a["weight"], a["kdeg"], n, nnz, sub, n_sub, gamma, two_m, a["comm"],
                                   a["tot"], a["size"], a["proposal"], None)


def modularity(lib, n=10, nnz=20, gamma=1.0, two_m=8.0, **p):
    a = {name: FAKE for name in ("indptr", "indices", "weight", "self_weight", "comm", "tot", "in_c", "q")}
    a.update(p)
    return lib.segger_louvain_modularity(a["indptr"], a["indices"], a["weight"], a["self_weight"], a["comm"], a["tot"], n, nnz,
                                         gamma, two_m, a["in_c"], a["q"], None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_knn_bruteforce_slabs": (i64, [i64, i32, i32]),
            "segger_knn_bruteforce_workspace_bytes": (i64, [i64, i32, i32]),
            "segger_knn_bruteforce": (C.c_int, [vp, i64, i32, i32, vp, vp, vp, i64, vp]),
            "segger_jaccard_weights": (C.c_int, [vp, vp, i64, i64, vp, vp]),
            "segger_louvain_move": (C.c_int, [vp, vp, vp, vp, i64, i64, i32, i32, f64, f64, vp, vp, vp, vp, vp]),
            "segger_louvain_modularity": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i64, f64, f64, vp, vp, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    import segger_amd
    from segger_amd import features, phenograph
    for name in ("knn_bruteforce", "jaccard_graph", "louvain"):
        assert getattr(segger_amd, name) is getattr(phenograph, name)
    assert segger_amd.phenograph is phenograph and callable(phenograph.phenograph)
    assert segger_amd.anndata_features is features.anndata_features


def test_slabs_and_workspace_are_functions_of_the_shapes(lib):
    slabs, ws = lib.segger_knn_bruteforce_slabs, lib.segger_knn_bruteforce_workspace_bytes
    assert [slabs(n, 16, 1) for n in (1, 127, 128, 255, 256, 300, 1000, 4096, 10 ** 5, 10 ** 6)] == [1, 1, 1, 1, 2, 2, 6, 16, 1, 1]
    assert slabs(1000, 1, 1) == slabs(1000, 256, 64) == 6              # n alone decides
    assert slabs(8192, 16, 1) <= _lib.KNN_BF_MAX_SLABS
    for n, d, k in ((1, 1, 1), (300, 128, 10), (1000, 256, 64), (10 ** 6, 128, 10), (1 << 30, 128, 64)):
        assert ws(n, d, k) == -(-n * 4 // 256) * 256 + slabs(n, d, k) * n * k * 8 > 0
    sizes = [ws(n, 128, 10) for n in (10, 100, 128, 129, 1000, 5000, 10 ** 5, 10 ** 6)]
    assert sizes == sorted(sizes) and [ws(1000, 8, k) for k in (1, 2, 64)] == sorted(ws(1000, 8, k) for k in (1, 2, 64))
    assert ws(1 << 30, 128, 64) > 1 << 39                              # n * k past 2^31: 64-bit sizes
    for fn in (slabs, ws):
        assert fn(0, 8, 1) == EINVAL and b"n must be" in lib.segger_last_error()
        assert fn(1 << 31, 8, 1) == EINVAL and b"2^31" in lib.segger_last_error()
        assert fn(10, 0, 1) == EINVAL and b"d = " in lib.segger_last_error()
        assert fn(10, _lib.KNN_BF_MAX_D + 1, 1) == EINVAL and b"d = " in lib.segger_last_error()
        assert fn(100, 8, 0) == EINVAL and b"k = " in lib.segger_last_error()
        assert fn(100, 8, _lib.KNN_BF_MAX_K + 1) == EINVAL and b"k = " in lib.segger_last_error()
        assert fn(5, 8, 6) == EINVAL and b"above n" in lib.segger_last_error()


def test_knn_rejections(lib):
    assert knn(lib, n=0) == EINVAL and b"n must be" in lib.segger_last_error()
    assert knn(lib, d=257) == EINVAL and b"d = 257" in lib.segger_last_error()
    assert knn(lib, k=65) == EINVAL and b"k = 65" in lib.segger_last_error()
    assert knn(lib, n=4, k=5) == EINVAL and b"above n" in lib.segger_last_error()
    for name in ("X", "idx", "dist2", "ws"):
        assert knn(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    for name in ("X", "idx", "dist2"):
        assert knn(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in lib.segger_last_error(), name
    assert knn(lib, ws=FAKE + 64) == EINVAL and b"256-byte aligned" in lib.segger_last_error()
    assert knn(lib, ws_bytes=-1) == EINVAL and b"workspace_bytes" in lib.segger_last_error()
    need = lib.segger_knn_bruteforce_workspace_bytes(100, 8, 5)
    assert knn(lib, ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.segger_last_error()


def test_graph_entry_rejections(lib):
    jac = lib.segger_jaccard_weights
    assert jac(FAKE, FAKE, -1, 4, FAKE, None) == EINVAL and b"negative n" in lib.segger_last_error()
    assert jac(FAKE, FAKE, 4, -1, FAKE, None) == EINVAL and b"nnz" in lib.segger_last_error()
    assert jac(None, FAKE, 4, 4, FAKE, None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert jac(FAKE, None, 4, 4, FAKE, None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert jac(FAKE, FAKE, 4, 4, None, None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert jac(FAKE + 4, FAKE, 4, 4, FAKE, None) == EINVAL and b"aligned" in lib.segger_last_error()
    assert jac(FAKE, FAKE, 4, 4, FAKE + 4, None) == EINVAL and b"aligned" in lib.segger_last_error()
    assert jac(FAKE, None, 4, 0, None, None) == 0                      # no edges: nothing to do, nothing launched
    assert move(lib, sub=4) == EINVAL and b"sub" in lib.segger_last_error()
    assert move(lib, n_sub=0) == EINVAL and b"n_sub" in lib.segger_last_error()
    assert move(lib, two_m=0.0) == EINVAL and b"two_m" in lib.segger_last_error()
    assert move(lib, gamma=-1.0) == EINVAL and b"gamma" in lib.segger_last_error()
    for name in ("indptr", "indices", "weight", "kdeg", "comm", "tot", "size", "proposal"):
        assert move(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    assert move(lib, tot=FAKE + 4) == EINVAL and b"aligned" in lib.segger_last_error()
    assert move(lib, n=0, nnz=0, indices=None, kdeg=None) == 0         # no vertices: nothing launched
    assert modularity(lib, two_m=-1.0) == EINVAL and b"two_m" in lib.segger_last_error()
    for name in ("indptr", "indices", "weight", "self_weight", "comm", "tot", "in_c", "q"):
        assert modularity(lib, **{name: None}) == EINVAL and b"NULL" in lib.segger_last_error(), name
    assert modularity(lib, q=FAKE + 4) == EINVAL and b"aligned" in lib.segger_last_error()


def test_python_side_rejects_cpu_tensors_and_bad_sizes():
    from segger_amd import phenograph as pg
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        pg.knn_bruteforce(torch.zeros(10, 4), 2)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        pg.jaccard_graph(torch.zeros(4, 2, dtype=torch.int32))
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        pg.phenograph(torch.zeros(10, 4), 2)
    # the relabelling is plain torch and runs anywhere
    got = pg.relabel_by_size(torch.tensor([5, 5, 2, 2, 9, 9, 9, 7]), 1)
    assert got.tolist() == [1, 1, 2, 2, 0, 0, 0, -1]
