"""Host layer of the GATv2 entry points (CPU): what segger_gatv2_fwd / _fwd_pair / _bwd / _bwd_pair, segger_dropout_bits
and segger_dropout_bits_many reject before they touch the device, with which code and which words in
segger_last_error().  Every device pointer is a fake aligned address that is never dereferenced, the stream is NULL and
every call below fails a host check: nothing is launched, zero-filled or memset (no backward without destinations, no
one-pass backward that still has to zero grad_xl, no generic destination pass).  Each input fails exactly one check."""
import ctypes as C

import pytest

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4                            # include/segger_amd.h
F32, BF16, F16 = 0, 1, 2
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
OTHER = 0x2000
H, CH = 2, 64                     # a specialised geometry
HC = H * CH
GH, GCH = 5, 24                   # a generic one: no vector loads, no alignment requirement
N_DST, N_SRC, N_EDGES = 10, 20, 30
BIG = 1 << 40                     # workspace_bytes that is never short


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _fill(a, f):
    """by_dst__x / by_src__x set a field of that view, everything else a field of the arguments"""
    for name, v in f.items():
        view, _, field = name.partition("__")
        setattr(getattr(a, view) if field else a, field or view, v)
    return a


def _csr(g, n_rows, n_cols):
    g.indptr, g.col, g.eid, g.n_rows, g.n_cols, g.n_edges = FAKE, FAKE, FAKE, n_rows, n_cols, N_EDGES


def fwd_args(heads=H, channels=CH, **f):
    a, hc = _lib.GatFwdArgs(), heads * channels
    _csr(a.by_dst, N_DST, N_SRC)
    a.x_l, a.ld_xl, a.x_r, a.ld_xr, a.att, a.bias = FAKE, hc, FAKE, hc, FAKE, FAKE
    a.heads, a.channels, a.dtype, a.apply_gelu, a.negative_slope = heads, channels, BF16, 1, 0.2
    a.out, a.ld_out, a.pre, a.ld_pre, a.lse = FAKE, hc, OTHER, hc, FAKE
    return _fill(a, f)


def bwd_args(heads=H, channels=CH, **f):
    a, hc = _lib.GatBwdArgs(), heads * channels
    _csr(a.by_dst, N_DST, N_SRC)
    _csr(a.by_src, N_SRC, N_DST)
    a.x_l, a.ld_xl, a.x_r, a.ld_xr, a.att, a.bias = FAKE, hc, FAKE, hc, FAKE, FAKE
    a.heads, a.channels, a.dtype, a.apply_gelu, a.negative_slope = heads, channels, BF16, 1, 0.2
    a.grad_out, a.ld_go, a.pre, a.ld_pre, a.lse = FAKE, hc, FAKE, hc, FAKE
    a.grad_pre, a.ld_gp, a.dsum = FAKE, hc, FAKE
    a.grad_xl, a.ld_gxl, a.grad_xr, a.ld_gxr, a.grad_att, a.grad_bias = FAKE, hc, FAKE, hc, FAKE, FAKE
    a.workspace, a.workspace_bytes = FAKE, BIG
    return _fill(a, f)


def fwd(lib, **f):
    return lib.segger_gatv2_fwd(C.byref(fwd_args(**f)), None)


def bwd(lib, **f):
    return lib.segger_gatv2_bwd(C.byref(bwd_args(**f)), None)


def fwd_second(lib, **f):                              # the second edge type of a pair; the first one is valid
    return lib.segger_gatv2_fwd_pair(C.byref(fwd_args()), C.byref(fwd_args(**f)), None)


def bwd_second(lib, **f):
    return lib.segger_gatv2_bwd_pair(C.byref(bwd_args()), C.byref(bwd_args(**f)), None)


def fwd_first(lib, **f):
    return lib.segger_gatv2_fwd_pair(C.byref(fwd_args(**f)), C.byref(fwd_args()), None)


def bwd_first(lib, **f):
    return lib.segger_gatv2_bwd_pair(C.byref(bwd_args(**f)), C.byref(bwd_args()), None)


FWD_CALLS = (fwd, fwd_first, fwd_second)
BWD_CALLS = (bwd, bwd_first, bwd_second)
# what is refused only behind the checks of BOTH edge types (passes, the storage type) cannot sit in a pair's second
# argument here: its valid first one would be launched before
FWD_LATE, BWD_LATE = (fwd, fwd_first), (bwd, bwd_first)


def check_csr(lib, call, view, **base):
    err = lib.segger_last_error
    v, who = view.encode(), (call.__name__, view)
    for size in ("n_rows", "n_cols", "n_edges"):
        assert call(lib, **{view + "__" + size: -1}, **base) == EINVAL and b"gatv2: negative size in " + v in err(), who
        assert call(lib, **{view + "__" + size: 0x7fffffff}, **base) == EINVAL, who
        assert b"gatv2: " + v + b" exceeds 2^31-1 rows/cols/edges" in err(), who
    assert call(lib, **{view + "__indptr": None}, **base) == EINVAL and b"gatv2: " + v + b".indptr is NULL" in err(), who
    assert call(lib, **{view + "__col": None}, **base) == EINVAL and b"gatv2: " + v + b".col is NULL" in err(), who


def check_rows(lib, call, name, ld, **base):
    """the five refusals of one matrix of a specialised geometry, bf16 and fp32"""
    err, n, who = lib.segger_last_error, name.encode(), (call.__name__, name)
    assert call(lib, **{name: None}, **base) == EINVAL and b"gatv2: " + n + b" is NULL" in err(), who
    assert call(lib, **{ld: HC - 1}, **base) == EINVAL and b"gatv2: ld of " + n + b" (127) < heads*channels (128)" in err(), who
    assert call(lib, **{ld: 1 << 31}, **base) == EINVAL and b"gatv2: row stride of " + n + b" exceeds 4 GiB" in err(), who
    assert call(lib, dtype=F32, **{ld: 1 << 30}, **base) == EINVAL and b"row stride of " + n + b" exceeds 4 GiB" in err(), who
    for off in (2, 4, 8):
        assert call(lib, **{name: FAKE + off}, **base) == EINVAL and b"gatv2: " + n + b" is not 16-byte aligned" in err(), who
    for dtype, bad in ((BF16, HC + 4), (F16, HC + 1), (F32, HC + 2)):
        assert call(lib, dtype=dtype, **{ld: bad}, **base) == EINVAL, who
        assert b"gatv2: row stride of " + n + b" is not a multiple of 16 bytes" in err(), who


def test_fwd_scalars_and_graph(lib):
    err = lib.segger_last_error
    assert lib.segger_gatv2_fwd(None, None) == EINVAL and b"segger_gatv2_fwd: args is NULL" in err()
    assert lib.segger_gatv2_fwd_pair(None, C.byref(fwd_args()), None) == EINVAL and b"segger_gatv2_fwd: args is NULL" in err()
    assert lib.segger_gatv2_fwd_pair(C.byref(fwd_args()), None, None) == EINVAL and b"segger_gatv2_fwd: args is NULL" in err()
    for call in FWD_CALLS:
        who = call.__name__
        for bad in (dict(heads=0), dict(channels=0), dict(heads=-1)):
            assert call(lib, **bad) == EINVAL and b"segger_gatv2_fwd: heads/channels must be positive" in err(), (who, bad)
        check_csr(lib, call, "by_dst")
        assert call(lib, att=None) == EINVAL and b"segger_gatv2_fwd: att is NULL" in err(), who
        for slope in (-0.1, 1.5):
            assert call(lib, negative_slope=slope) == EINVAL and b"segger_gatv2_fwd: negative_slope must be in [0,1]" in err(), who
        for p in (-0.1, 1.0):
            assert call(lib, dropout_p=p) == EINVAL and b"segger_gatv2_fwd: dropout_p must be in [0,1)" in err(), who


def test_fwd_matrices(lib):
    err = lib.segger_last_error
    for call in FWD_CALLS:
        for name, ld in (("x_r", "ld_xr"), ("out", "ld_out"), ("x_l", "ld_xl")):
            check_rows(lib, call, name, ld)
        # pre is optional: NULL is no refusal
        assert call(lib, ld_pre=HC - 1) == EINVAL and b"gatv2: ld of pre (127) < heads*channels (128)" in err()
        assert call(lib, ld_pre=1 << 31) == EINVAL and b"gatv2: row stride of pre exceeds 4 GiB" in err()
        assert call(lib, pre=OTHER + 8) == EINVAL and b"gatv2: pre is not 16-byte aligned" in err()
        assert call(lib, ld_pre=HC + 4) == EINVAL and b"gatv2: row stride of pre is not a multiple of 16 bytes" in err()
        assert call(lib, pre=FAKE) == EINVAL and b"segger_gatv2_fwd: pre may alias out only without GELU" in err()
        # x_l is not read without edges: its NULL passes, and the call fails a later check
        assert call(lib, by_dst__n_edges=0, x_l=None, pre=FAKE) == EINVAL and b"pre may alias out" in err()


def test_fwd_eid_rules(lib):
    err = lib.segger_last_error
    word = b"segger_gatv2_fwd: by_dst.eid is required for dropout (without keep_bits) / alpha output"
    for call in FWD_CALLS:
        assert call(lib, by_dst__eid=None, dropout_p=0.5) == EINVAL and word in err(), call.__name__
        assert call(lib, by_dst__eid=None, alpha=FAKE) == EINVAL and word in err(), call.__name__
        assert call(lib, by_dst__eid=None, alpha=FAKE, dropout_p=0.5, keep_bits=FAKE) == EINVAL and word in err(), call.__name__


def test_generic_geometry_takes_misaligned_rows(lib):
    """heads 5, channels 24 has no specialised kernel: element loads, so neither the row addresses nor the strides have to
    be multiples of 16 bytes -- the call gets past every matrix and fails the check behind them"""
    err = lib.segger_last_error
    g, ghc = dict(heads=GH, channels=GCH), GH * GCH
    odd = dict(x_r=FAKE + 2, x_l=FAKE + 6, ld_xr=ghc + 1, ld_xl=ghc + 3)
    for call in FWD_CALLS:
        assert call(lib, out=FAKE + 2, ld_out=ghc + 1, pre=FAKE + 2, ld_pre=ghc + 1, **odd, **g) == EINVAL, call.__name__
        assert b"pre may alias out only without GELU" in err(), call.__name__
        assert call(lib, ld_xr=ghc - 1, **g) == EINVAL and b"gatv2: ld of x_r (119) < heads*channels (120)" in err()
    odd.update(grad_out=FAKE + 2, ld_go=ghc + 1, pre=FAKE + 10, ld_pre=ghc + 5, grad_pre=FAKE + 2, ld_gp=ghc + 1,
               grad_xr=FAKE + 4, ld_gxr=ghc + 1, grad_xl=FAKE + 2, ld_gxl=ghc + 7)
    for call in BWD_LATE:
        assert call(lib, passes=4, **odd, **g) == EINVAL and b"segger_gatv2_bwd: passes must be" in err(), call.__name__
    for call in BWD_CALLS:
        assert call(lib, grad_xl=None, **g) == EINVAL and b"gatv2: grad_xl is NULL" in err(), call.__name__
        assert call(lib, src_unique=1, **g) == EINVAL, call.__name__
        assert b"segger_gatv2_bwd: src_unique needs a specialised (heads, channels) geometry" in err(), call.__name__
        assert call(lib, zero_rows_out=FAKE, ld_zero=ghc, **g) == EINVAL, call.__name__
        assert b"segger_gatv2_bwd: zero_rows_out needs the two-pass backward of a specialised geometry" in err(), call.__name__


def test_bwd_scalars_and_graphs(lib):
    err = lib.segger_last_error
    assert lib.segger_gatv2_bwd(None, None) == EINVAL and b"segger_gatv2_bwd: args is NULL" in err()
    assert lib.segger_gatv2_bwd_pair(None, C.byref(bwd_args()), None) == EINVAL and b"segger_gatv2_bwd: args is NULL" in err()
    assert lib.segger_gatv2_bwd_pair(C.byref(bwd_args()), None, None) == EINVAL and b"segger_gatv2_bwd: args is NULL" in err()
    for call in BWD_CALLS:
        who = call.__name__
        for bad in (dict(heads=0), dict(channels=0), dict(channels=-8)):
            assert call(lib, **bad) == EINVAL and b"segger_gatv2_bwd: heads/channels must be positive" in err(), (who, bad)
        check_csr(lib, call, "by_dst")
        check_csr(lib, call, "by_dst", src_unique=1)
        check_csr(lib, call, "by_src")
        word = b"segger_gatv2_bwd: by_dst and by_src describe different graphs"
        for bad in (dict(by_src__n_edges=N_EDGES + 1), dict(by_src__n_rows=N_SRC + 1), dict(by_src__n_cols=N_DST - 1),
                    dict(by_dst__n_rows=N_DST + 1), dict(by_dst__n_cols=0)):
            assert call(lib, **bad) == EINVAL and word in err(), (who, bad)
        # the one-pass form reads no by_src: a broken one is not looked at, and the call fails a later check
        assert call(lib, src_unique=1, by_src__indptr=None, by_src__n_edges=-1, att=None) == EINVAL and b"att / grad_att" in err()
        for name in ("att", "grad_att"):
            assert call(lib, **{name: None}) == EINVAL and b"segger_gatv2_bwd: att / grad_att is NULL" in err(), (who, name)
        for slope in (-0.1, 1.5):
            assert call(lib, negative_slope=slope) == EINVAL and b"segger_gatv2_bwd: negative_slope must be in [0,1]" in err(), who
        for p in (-0.1, 1.0):
            assert call(lib, dropout_p=p) == EINVAL and b"segger_gatv2_bwd: dropout_p must be in [0,1)" in err(), who


def test_bwd_matrices(lib):
    err = lib.segger_last_error
    for call in BWD_CALLS:
        for base in (dict(), dict(src_unique=1)):
            for name, ld in (("x_r", "ld_xr"), ("grad_out", "ld_go"), ("pre", "ld_pre"), ("grad_pre", "ld_gp"),
                             ("grad_xr", "ld_gxr"), ("x_l", "ld_xl"), ("grad_xl", "ld_gxl")):
                check_rows(lib, call, name, ld, **base)
            for name in ("lse", "dsum"):
                assert call(lib, **{name: None}, **base) == EINVAL and b"segger_gatv2_bwd: lse / dsum is NULL" in err(), name
        # the destination-side matrices come first, the source-side ones behind them
        assert call(lib, x_l=None, dsum=None) == EINVAL and b"lse / dsum is NULL" in err()
        assert call(lib, x_l=None, workspace=None) == EINVAL and b"gatv2: x_l is NULL" in err()


def test_bwd_eid_rules(lib):
    err = lib.segger_last_error
    word = b"segger_gatv2_bwd: eid arrays (or keep_bits) are required for dropout"
    for call in BWD_CALLS:
        assert call(lib, dropout_p=0.5, by_dst__eid=None) == EINVAL and word in err(), call.__name__
        assert call(lib, dropout_p=0.5, by_src__eid=None) == EINVAL and word in err(), call.__name__
        assert call(lib, dropout_p=0.5, by_dst__eid=None, keep_bits_src=FAKE) == EINVAL and word in err(), call.__name__
        assert call(lib, dropout_p=0.5, by_src__eid=None, keep_bits_dst=FAKE) == EINVAL and word in err(), call.__name__
        assert call(lib, dropout_p=0.5, by_dst__eid=None, src_unique=1) == EINVAL and word in err(), call.__name__
        # keep_bits stand in for eid, and the one-pass form needs nothing of by_src: these get to the next check
        ok = dict(dropout_p=0.5, workspace=None)
        assert call(lib, by_dst__eid=None, by_src__eid=None, keep_bits_dst=FAKE, keep_bits_src=FAKE, **ok) == EWORKSPACE
        assert call(lib, by_src__eid=None, src_unique=1, **ok) == EWORKSPACE


def test_bwd_workspace(lib):
    err = lib.segger_last_error
    for call in BWD_CALLS:
        for heads, channels in ((H, CH), (1, 32), (4, 64), (GH, GCH)):
            g = dict(heads=heads, channels=channels)
            want = lib.segger_gatv2_bwd_workspace_bytes_two_pass(N_DST, N_SRC, N_EDGES, heads, channels)
            assert call(lib, workspace_bytes=want - 1, **g) == EWORKSPACE, (call.__name__, g)
            assert err() == b"segger_gatv2_bwd: workspace %d < %d bytes" % (want - 1, want), (call.__name__, g)
            assert call(lib, workspace=None, **g) == EWORKSPACE and b"segger_gatv2_bwd: workspace" in err(), (call.__name__, g)
        # wave-per-row source pass (degree 32): four rows per block, a larger source slab
        want = lib.segger_gatv2_bwd_workspace_bytes_two_pass(N_DST, N_SRC, 32 * N_SRC, H, CH)
        assert want > lib.segger_gatv2_bwd_workspace_bytes_two_pass(N_DST, N_SRC, 32 * N_SRC - 1, H, CH)
        many = dict(by_dst__n_edges=32 * N_SRC, by_src__n_edges=32 * N_SRC)
        assert call(lib, workspace_bytes=want - 1, **many) == EWORKSPACE
        assert err() == b"segger_gatv2_bwd: workspace %d < %d bytes" % (want - 1, want)
        # the one-pass form has no source slab
        want = lib.segger_gatv2_bwd_workspace_bytes(N_DST, H, CH)
        assert want < lib.segger_gatv2_bwd_workspace_bytes_two_pass(N_DST, N_SRC, N_EDGES, H, CH)
        assert call(lib, src_unique=1, workspace_bytes=want - 1) == EWORKSPACE
        assert err() == b"segger_gatv2_bwd: workspace %d < %d bytes" % (want - 1, want)


def test_bwd_zero_rows_out_and_passes(lib):
    err = lib.segger_last_error
    for call in BWD_CALLS:
        who = call.__name__
        assert call(lib, zero_rows_out=FAKE, ld_zero=HC, src_unique=1) == EINVAL, who
        assert b"segger_gatv2_bwd: zero_rows_out needs the two-pass backward of a specialised geometry" in err(), who
        z = dict(zero_rows_out=FAKE)
        assert call(lib, ld_zero=HC - 1, **z) == EINVAL and b"gatv2: ld of zero_rows_out (127) < heads*channels (128)" in err(), who
        assert call(lib, ld_zero=1 << 31, **z) == EINVAL and b"gatv2: row stride of zero_rows_out exceeds 4 GiB" in err(), who
        assert call(lib, zero_rows_out=FAKE + 8, ld_zero=HC) == EINVAL and b"gatv2: zero_rows_out is not 16-byte aligned" in err()
        assert call(lib, ld_zero=HC + 4, **z) == EINVAL and b"row stride of zero_rows_out is not a multiple of 16 bytes" in err()
    for call in BWD_LATE:
        who = call.__name__
        for passes in (-1, 4, 7):
            assert call(lib, passes=passes) == EINVAL, (who, passes)
            assert b"segger_gatv2_bwd: passes must be 0 (both), 1 (destination), 2 (source) or 3" in err(), (who, passes)
            assert call(lib, passes=passes, zero_rows_out=FAKE, ld_zero=HC) == EINVAL and b"passes must be" in err(), (who, passes)


def test_unknown_dtype(lib):
    """refused with one message on every route that gets to its launch without a device call before it"""
    err = lib.segger_last_error
    word = b"gatv2: unknown dtype 3"
    generic = dict(heads=GH, channels=GCH)
    for call in FWD_LATE:
        assert call(lib, dtype=3) == EINVAL and word in err(), call.__name__
        assert call(lib, dtype=-1) == EINVAL and b"gatv2: unknown dtype -1" in err(), call.__name__
        assert call(lib, dtype=3, **generic) == EINVAL and word in err(), call.__name__
    # both edge types of a pair in an unknown type: the merged launch of a low-degree and a high-degree one, too
    for second in (dict(), dict(by_dst__n_edges=32 * N_DST)):
        a, b = fwd_args(dtype=3), fwd_args(dtype=3, **second)
        assert lib.segger_gatv2_fwd_pair(C.byref(a), C.byref(b), None) == EINVAL and word in err(), second
    for call in BWD_LATE:
        for passes in (0, 1, 2, 3):
            assert call(lib, dtype=3, passes=passes) == EINVAL and word in err(), (call.__name__, passes)
        assert call(lib, dtype=3, src_unique=1, grad_xl_zeroed=1) == EINVAL and word in err(), call.__name__
        assert call(lib, dtype=3, passes=2, **generic) == EINVAL and word in err(), call.__name__
    # the merged backward pair: a two-pass low-degree, b one-pass high-degree over a's destinations
    a = bwd_args(dtype=3, by_dst__n_cols=N_DST, by_src__n_rows=N_DST, grad_xl=OTHER)
    b = bwd_args(dtype=3, src_unique=1, by_dst__n_cols=N_DST, by_dst__n_edges=32 * N_DST)
    assert lib.segger_gatv2_bwd_pair(C.byref(a), C.byref(b), None) == EINVAL and word in err()


def bits(lib, **f):
    seeds = (C.c_uint64 * 16)(*range(16))
    a = dict(eid=FAKE, n_edges=100, heads=H, dropout_p=0.5, seeds=C.addressof(seeds), n_seeds=3, seed_dev=None, bits=FAKE,
             plane_stride=100)
    a.update(f)
    return lib.segger_dropout_bits(a["eid"], a["n_edges"], a["heads"], a["dropout_p"], a["seeds"], a["n_seeds"], a["seed_dev"],
                                   a["bits"], a["plane_stride"], None)


def bits_many(lib, n_jobs=2, heads=H, dropout_p=0.5, jobs=True, **last):
    """n_jobs jobs, the fields in `last` set on the last one"""
    seeds = (C.c_uint64 * 16)(*range(16))
    arr = (_lib.BitsJob * 4)()
    for j in arr:
        j.eid, j.n_edges, j.seeds, j.n_seeds, j.bits, j.plane_stride = FAKE, 100, C.addressof(seeds), 3, FAKE, 100
    _fill(arr[min(max(n_jobs, 1), 4) - 1], last)
    return lib.segger_dropout_bits_many(C.addressof(arr) if jobs else None, n_jobs, heads, dropout_p, None, None)


def test_dropout_bits(lib):
    err = lib.segger_last_error
    for bad in (dict(n_edges=-1), dict(heads=0), dict(heads=9)):
        assert bits(lib, **bad) == EINVAL and b"segger_dropout_bits: heads must be in 1..8" in err(), bad
    for bad in (dict(n_seeds=0), dict(n_seeds=17), dict(seeds=None)):
        assert bits(lib, **bad) == EINVAL and b"segger_dropout_bits: 1..16 seeds" in err(), bad
    for p in (-0.1, 1.0):
        assert bits(lib, dropout_p=p) == EINVAL and b"segger_dropout_bits: dropout_p must be in [0,1)" in err(), p
    for name in ("eid", "bits"):
        assert bits(lib, **{name: None}) == EINVAL and b"segger_dropout_bits: NULL pointer" in err(), name
    word = b"segger_dropout_bits: plane_stride must be a multiple of 4 >= n_edges"
    for bad in (dict(plane_stride=96), dict(plane_stride=102), dict(bits=FAKE + 2)):
        assert bits(lib, **bad) == EINVAL and word in err() and b"bits 4-byte aligned" in err(), bad
    assert bits(lib, n_edges=0, eid=None, bits=None, plane_stride=3) == 0            # nothing to draw: nothing launched


def test_dropout_bits_many(lib):
    err = lib.segger_last_error
    for bad in (dict(jobs=False), dict(n_jobs=0), dict(n_jobs=5), dict(n_jobs=-1)):
        assert bits_many(lib, **bad) == EINVAL and b"segger_dropout_bits_many: 1..4 jobs" in err(), bad
    for heads in (0, 9):
        assert bits_many(lib, heads=heads) == EINVAL and b"segger_dropout_bits_many: heads must be in 1..8" in err(), heads
    for p in (-0.1, 1.0):
        assert bits_many(lib, dropout_p=p) == EINVAL and b"segger_dropout_bits_many: dropout_p must be in [0,1)" in err(), p
    for n_jobs in (1, 2, 4):
        job = b"segger_dropout_bits_many: job %d: " % (n_jobs - 1)
        for bad in (dict(n_edges=-1), dict(n_seeds=0), dict(n_seeds=17)):
            assert bits_many(lib, n_jobs, **bad) == EINVAL and job + b"bad sizes" in err(), (n_jobs, bad)
        for name in ("eid", "bits"):
            assert bits_many(lib, n_jobs, **{name: None}) == EINVAL and job + b"NULL pointer" in err(), (n_jobs, name)
        for bad in (dict(plane_stride=96), dict(plane_stride=102), dict(bits=FAKE + 2)):
            assert bits_many(lib, n_jobs, **bad) == EINVAL, (n_jobs, bad)
            assert job + b"plane_stride must be a multiple of 4 >= n_edges" in err() and b"bits 4-byte aligned" in err()
        # an empty job still has its stride looked at
        assert bits_many(lib, n_jobs, n_edges=0, eid=None, plane_stride=2) == EINVAL and job + b"plane_stride must be" in err()
    empty = (_lib.BitsJob * 4)()
    seeds = (C.c_uint64 * 16)()
    for j in empty:
        j.seeds, j.n_seeds = C.addressof(seeds), 1
    assert lib.segger_dropout_bits_many(C.addressof(empty), 4, H, 0.5, None, None) == 0   # nothing to draw
