"""C-ABI surface of the contamination entry points (CPU): the symbols exist with the documented signatures, the ABI
version is still 32, bad arguments are rejected on the host with SEGGER_EINVAL and a message, and empty inputs return 0
-- nothing is launched by any call below (every pointer is a fake aligned address that is never dereferenced)."""
import ctypes as C
import math

import pytest
import torch

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double

FREQ_PTRS = ("nbr", "dist", "labels", "counts", "freq")
POST_IN = ("indptr", "indices", "counts", "gene_map", "host_type", "freq", "Lt", "back")
POST_OUT = ("q_self", "q_neighbor", "q_background", "contamination", "contaminated", "total", "percent")
POST_8 = ("indptr", "back", "contaminated", "total", "percent")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def freq(lib, n=10, k=5, T=3, max_distance=math.inf, **p):
    a = {name: FAKE for name in FREQ_PTRS}
    a.update(p)
    return lib.segger_neighbor_frequencies(a["nbr"], a["dist"], a["labels"], n, k, T, max_distance, a["counts"], a["freq"], None)


def post(lib, n=10, n_cols=8, nnz=20, ld=4, T=3, G=7, a_s=0.8, a_n=0.15, a_b=0.05, eps=1e-6, cutoff=0.5, **p):
    a = {name: FAKE for name in POST_IN + POST_OUT}
    a.update(p)
    return lib.segger_contamination_posterior(a["indptr"], a["indices"], a["counts"], n, n_cols, nnz, a["gene_map"], a["host_type"],
                                              a["freq"], a["Lt"], ld, a["back"], T, G, a_s, a_n, a_b, eps, cutoff, a["q_self"],
                                              a["q_neighbor"], a["q_background"], a["contamination"], a["contaminated"], a["total"],
                                              a["percent"], None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_neighbor_frequencies": (C.c_int, [vp, vp, vp, i64, i32, i32, f64, vp, vp, vp]),
            "segger_contamination_posterior": (C.c_int, [vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, i64, vp, i32, i32, f64, f64, f64,
                                                         f64, f64, vp, vp, vp, vp, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    assert (_lib.CONTAM_MAX_TYPES, _lib.CONTAM_MAX_K) == (256, 64)
    import segger_amd
    from segger_amd import validation
    assert segger_amd.validation is validation
    for name in ("neighbor_frequencies", "reference_table", "calculate_contamination", "contamination_flow"):
        assert getattr(segger_amd, name) is getattr(validation, name)


def test_neighbor_frequencies_rejections(lib):
    err = lib.segger_last_error
    assert freq(lib, n=-1) == EINVAL and b"negative n" in err()
    assert freq(lib, n=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    for k in (0, -1, 65):
        assert freq(lib, k=k) == EINVAL and b"k = " in err(), k
    for T in (0, -3, 257):
        assert freq(lib, T=T) == EINVAL and b"n_types = " in err(), T
    for md in (math.nan, -1.0, -math.inf):
        assert freq(lib, max_distance=md) == EINVAL and b"max_distance" in err(), md
    for name in FREQ_PTRS:
        assert freq(lib, **{name: None}) == EINVAL and b"NULL" in err(), name
        assert freq(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in err(), name
    assert freq(lib, n=0, nbr=None, dist=None, labels=None, counts=None, freq=None) == 0      # no points: nothing launched


def test_contamination_posterior_rejections(lib):
    err = lib.segger_last_error
    assert post(lib, n=-1) == EINVAL and b"negative" in err()
    assert post(lib, n_cols=-1) == EINVAL and b"negative" in err()
    assert post(lib, nnz=-1) == EINVAL and b"nnz" in err()
    assert post(lib, n=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    for T in (0, -1, 257):
        assert post(lib, T=T, ld=260) == EINVAL and b"n_types = " in err(), T
    for G in (0, -1, _lib.CONTAM_MAX_REF_GENES + 1):
        assert post(lib, G=G) == EINVAL and b"n_ref_genes = " in err(), G
    for ld in (0, 2, 3, 6, -4):                                          # below n_types, or no multiple of 4
        assert post(lib, ld=ld) == EINVAL and b"ld_L" in err(), ld
    for bad in (math.nan, math.inf, -math.inf):
        for name in ("a_s", "a_n", "a_b"):
            assert post(lib, **{name: bad}) == EINVAL and b"alpha" in err(), (name, bad)
        assert post(lib, eps=bad) == EINVAL and b"eps" in err(), bad
    assert post(lib, cutoff=math.nan) == EINVAL and b"cutoff" in err()
    assert post(lib, n_cols=0) == EINVAL and b"n_cols" in err()
    for name in POST_IN + POST_OUT:
        assert post(lib, **{name: None}) == EINVAL and b"NULL" in err(), name
        assert post(lib, **{name: FAKE + 2}) == EINVAL and b"aligned" in err(), name
    for name in POST_8:
        assert post(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    assert post(lib, Lt=FAKE + 8) == EINVAL and b"16-byte aligned" in err()
    none = {name: None for name in POST_IN + POST_OUT}
    assert post(lib, n=0, nnz=0, **none) == 0                           # no rows: nothing launched
    assert post(lib, nnz=0, **none) == 0                                # no stored entries: nothing launched, nothing written


def test_python_side_rejects_cpu_tensors():
    from segger_amd import validation as va
    i32t = dict(dtype=torch.int32)
    expr = {"indptr": torch.zeros(3, dtype=torch.int64), "indices": torch.zeros(0, **i32t), "counts": torch.zeros(0, **i32t),
            "gene_ids": torch.zeros(4, **i32t), "centroid": torch.zeros(2, 2, dtype=torch.float64)}
    kind, weight = torch.zeros(2, **i32t), torch.ones(2, 4, dtype=torch.float64)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        va.neighbor_frequencies(torch.zeros(5, 2), torch.zeros(5, **i32t), 2, 3)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        va.reference_table(expr["indptr"], expr["indices"], expr["counts"], kind, 2)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        va.calculate_contamination(expr, kind, weight)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        va.contamination_flow(expr, expr["counts"], kind, weight)
    with pytest.raises(ValueError, match="centroid"):
        va.calculate_contamination({k: v for k, v in expr.items() if k != "centroid"}, kind, weight)
