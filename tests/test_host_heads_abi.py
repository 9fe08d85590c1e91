"""Host layer of the scoring heads (CPU): what segger_triplet_fwd / _bwd (both loss kinds), segger_metric_fwd / _bwd,
segger_edge_cos_argmax and the three segger_loss_combine_* entries reject before they touch the device, with which code
and which words in segger_last_error(), plus the literal values of segger_triplet_partial_count and
segger_triplet_workspace_bytes.  Every device pointer is a fake aligned address that is never dereferenced, the stream is
NULL and every call below fails a host check: nothing is launched and nothing is zeroed (no call with n_edges = 0 and a
loss pointer, no call with every argument valid).  Each input fails exactly one check."""
import ctypes as C

import pytest

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4                            # include/segger_amd.h
F32, BF16, F16 = 0, 1, 2
TRIPLET, BCE = 0, 1                                    # SEGGER_LOSS_*
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
OTHER = 0x2000                    # a second one: grad_b apart from grad_a
N, NB, CH = 100, 10, 64           # triplets (= rows of z_a), rows of z_b, channels
BIG = 1 << 40                     # workspace_bytes that is never short


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def args(kind=TRIPLET, **f):
    a = _lib.TripletArgs()
    a.src, a.pos, a.neg, a.n_edges = FAKE, FAKE, FAKE, N
    a.z_a, a.ld_za, a.n_a, a.z_b, a.ld_zb, a.n_b = FAKE, CH, N, FAKE, CH, NB
    a.channels, a.dtype, a.margin, a.eps, a.loss_kind = CH, BF16, 0.4, 1e-6, kind
    a.loss, a.workspace, a.workspace_bytes = FAKE, FAKE, BIG
    a.grad_scale, a.grad_a, a.grad_b = 1.0, FAKE, OTHER
    for name, v in f.items():
        setattr(a, name, v)
    return a


def fwd(lib, kind=TRIPLET, **f):
    return lib.segger_triplet_fwd(C.byref(args(kind, **f)), None)


def bwd(lib, kind=TRIPLET, **f):
    return lib.segger_triplet_bwd(C.byref(args(kind, **f)), None)


GROUPS = dict(pos_indptr=FAKE, pos_eid=FAKE)            # the triplets grouped by positive row
WALK = dict(GROUPS, anchor_unique=1)                   # ... and unique anchors: the one-walk routes


def metric_fwd(lib, n=N, c=CH, ld=CH, dtype=BF16, ws_bytes=BIG, **p):
    a = dict(z=FAKE, pos=FAKE, neg=FAKE, d_pos=FAKE, d_neg=FAKE, w=FAKE, loss=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_metric_fwd(a["z"], ld, n, c, dtype, a["pos"], a["neg"], a["d_pos"], a["d_neg"], a["w"], 1e-8, a["loss"],
                                 a["workspace"], ws_bytes, None)


def metric_bwd(lib, n=N, c=CH, ld=CH, dtype=BF16, **p):
    a = dict(z=FAKE, pos=FAKE, neg=FAKE, d_pos=FAKE, d_neg=FAKE, w=FAKE, scale=FAKE, grad_z=FAKE)
    a.update(p)
    return lib.segger_metric_bwd(a["z"], ld, n, c, dtype, a["pos"], a["neg"], a["d_pos"], a["d_neg"], a["w"], 1e-8, a["scale"],
                                 a["grad_z"], None)


def argmax(lib, n_rows=N, n_cols=NB, n_edges=300, **f):
    a = _lib.EdgeArgmaxArgs()
    g = a.by_src
    g.indptr, g.col, g.eid, g.n_rows, g.n_cols, g.n_edges = FAKE, FAKE, FAKE, n_rows, n_cols, n_edges
    a.z_src, a.ld_zs, a.z_dst, a.ld_zd, a.channels, a.dtype, a.eps = FAKE, CH, FAKE, CH, CH, BF16, 1e-8
    a.max_sim, a.max_eid, a.seg_idx = FAKE, FAKE, FAKE
    for name, v in f.items():
        setattr(g if name in ("indptr", "col") else a, name, v)
    return lib.segger_edge_cos_argmax(C.byref(a), None)


def test_triplet_sizes_and_inputs(lib):
    err = lib.segger_last_error
    for call in (fwd, bwd):
        for kind in (TRIPLET, BCE):
            who = (call.__name__, kind)
            assert getattr(lib, "segger_triplet_" + call.__name__)(None, None) == EINVAL and b"args is NULL" in err()
            assert call(lib, kind, n_edges=-1) == EINVAL and b"bad sizes" in err(), who
            assert call(lib, kind, channels=0) == EINVAL and b"bad sizes" in err(), who
            assert call(lib, kind, n_edges=0x7fffffff * 64) == EINVAL and b"too many edges" in err(), who
            for name in ("src", "pos", "neg", "z_a", "z_b"):
                assert call(lib, kind, **{name: None}) == EINVAL and b"NULL input" in err(), (who, name)
            for name in ("ld_za", "ld_zb"):
                assert call(lib, kind, **{name: CH - 2}) == EINVAL and b"ld < channels" in err(), (who, name)
            for name in ("n_a", "n_b"):
                assert call(lib, kind, **{name: 0}) == EINVAL and b"must be positive" in err(), (who, name)
            assert call(lib, kind, dtype=3) == EINVAL and b"segger_triplet: unknown dtype 3" in err(), who
    assert bwd(lib, TRIPLET, dtype=3, **WALK) == EINVAL and b"segger_triplet: unknown dtype 3" in err()
    assert bwd(lib, BCE, dtype=3, **WALK) == EINVAL and b"segger_triplet: unknown dtype 3" in err()
    assert bwd(lib, TRIPLET, dtype=3, **GROUPS) == EINVAL and b"segger_triplet: unknown dtype 3" in err()


def test_triplet_fwd_workspace(lib):
    err = lib.segger_last_error
    for kind in (TRIPLET, BCE):
        for n in (1, 64, 65, N):
            want = lib.segger_triplet_workspace_bytes(n)
            assert fwd(lib, kind, n_edges=n, workspace_bytes=want - 1) == EWORKSPACE, (kind, n)
            assert err() == b"segger_triplet_fwd: workspace %d < %d bytes" % (want - 1, want), (kind, n)
        assert fwd(lib, kind, workspace=None) == EWORKSPACE and b"segger_triplet_fwd: workspace" in err(), kind


def test_triplet_bwd_gradient_buffers(lib):
    err = lib.segger_last_error
    for kind in (TRIPLET, BCE):
        assert bwd(lib, kind, grad_a=None) == EINVAL and b"NULL gradient buffer" in err(), kind
        assert bwd(lib, kind, grad_b=None) == EINVAL and b"NULL gradient buffer" in err(), kind
        # packed 16-bit atomics: a 16-bit dtype, an even channel count (odd counts: the triplet loss only, the BCE head
        # refuses them by itself), one layout per buffer
        for f in (dict(grad_a_packed=1), dict(grad_b_packed=1), dict(grad_a_packed=1, grad_b_packed=1)):
            assert bwd(lib, kind, dtype=F32, **f) == EINVAL and b"packed gradient buffers" in err(), (kind, f)
        for f in (dict(grad_a_packed=1), dict(grad_b_packed=1)):
            assert bwd(lib, kind, grad_b=FAKE, **f) == EINVAL and b"one shared gradient buffer" in err(), (kind, f)
    for dtype in (BF16, F16):
        assert bwd(lib, channels=21, ld_za=21, ld_zb=21, dtype=dtype, grad_a_packed=1) == EINVAL and b"packed gradient" in err()


def test_triplet_bwd_contrib(lib):
    err = lib.segger_last_error
    assert bwd(lib, contrib=FAKE, channels=21, ld_za=21, ld_zb=21) == EINVAL and b"contrib needs an even channel count" in err()
    assert bwd(lib, contrib=FAKE, grad_b=FAKE) == EINVAL and b"contrib needs" in err() and b"separate z_b" in err()
    assert bwd(lib, BCE, contrib=FAKE) == EINVAL and b"(BCE): contrib is a triplet-loss option" in err()
    assert bwd(lib, BCE, contrib=FAKE, grad_b=None) == EINVAL and b"(BCE): contrib is a triplet-loss option" in err()


def test_triplet_bwd_grad_a_rows(lib):
    err = lib.segger_last_error
    word = b"grad_a_rows needs"
    assert bwd(lib, grad_a_rows=FAKE, channels=21, ld_za=21, ld_zb=21) == EINVAL and word in err()
    assert bwd(lib, grad_a_rows=FAKE, n_edges=N - 1) == EINVAL and word in err()
    assert bwd(lib, grad_a_rows=FAKE, n_a=N + 1) == EINVAL and word in err()
    assert bwd(lib, grad_a_rows=FAKE + 4) == EINVAL and word in err()
    assert bwd(lib, BCE, grad_a_rows=FAKE) == EINVAL and word in err()


def test_triplet_bwd_groups_by_positive_row(lib):
    err = lib.segger_last_error
    word = b"pos_indptr needs pos_eid and a separate fp32 grad_b"
    for kind in (TRIPLET, BCE):
        for unique in (0, 1):
            kw = dict(pos_indptr=FAKE, pos_eid=FAKE, anchor_unique=unique)
            assert bwd(lib, kind, **dict(kw, pos_eid=None)) == EINVAL and word in err(), (kind, unique)
            assert bwd(lib, kind, grad_b=FAKE, **kw) == EINVAL and word in err(), (kind, unique)
            assert bwd(lib, kind, grad_b_packed=1, **kw) == EINVAL and word in err(), (kind, unique)


def test_bce_alignment(lib):
    err = lib.segger_last_error
    word = b"segger_triplet (BCE): even channel count and 8-byte aligned rows"
    for call in (fwd, bwd):
        assert call(lib, BCE, channels=21, ld_za=22, ld_zb=22) == EINVAL and word in err(), call.__name__
        for name in ("z_a", "z_b"):
            assert call(lib, BCE, **{name: FAKE + 4}) == EINVAL and word in err(), (call.__name__, name)
        for name in ("ld_za", "ld_zb"):                # 16-bit rows must start on 4 bytes: an even leading dimension
            assert call(lib, BCE, **{name: CH + 1}) == EINVAL and word in err(), (call.__name__, name)
            assert call(lib, BCE, dtype=F16, **{name: CH + 1}) == EINVAL and word in err(), (call.__name__, name)
        assert call(lib, BCE, n_b=1 << 31) == EINVAL and b"segger_triplet (BCE): too many rows in z_b" in err(), call.__name__
    assert bwd(lib, BCE, n_b=1 << 31, **WALK) == EINVAL and b"segger_triplet (BCE): too many rows in z_b" in err()


def test_triplet_one_walk_route(lib):
    err = lib.segger_last_error
    word = b"segger_triplet_bwd: anchor_unique needs C in {32, 64, 96, 128} and 8-byte aligned rows"
    for c in (16, 48, 160, 256):
        assert bwd(lib, channels=c, ld_za=c, ld_zb=c, **WALK) == EINVAL and word in err(), c
    for name in ("z_a", "z_b", "grad_a"):
        assert bwd(lib, **{name: FAKE + 4}, **WALK) == EINVAL and word in err(), name
    for dtype in (BF16, F16):
        for name in ("ld_za", "ld_zb"):
            assert bwd(lib, dtype=dtype, **{name: CH + 1}, **WALK) == EINVAL and word in err(), (dtype, name)
    assert bwd(lib, n_b=1 << 31, **WALK) == EINVAL and b"segger_triplet_bwd: too many rows in z_b" in err()


def test_metric(lib):
    err = lib.segger_last_error
    for call in (metric_fwd, metric_bwd):
        for bad in (dict(n=-1), dict(c=0), dict(ld=CH - 1)):
            assert call(lib, **bad) == EINVAL and b"segger_metric: bad sizes" in err(), (call.__name__, bad)
        for name in ("z", "pos", "neg", "d_pos", "d_neg", "w"):
            assert call(lib, **{name: None}) == EINVAL and b"segger_metric: NULL input" in err(), (call.__name__, name)
        assert call(lib, dtype=3) == EINVAL and b"segger_metric: unknown dtype 3" in err(), call.__name__
    for n in (1, 64, 65, N):
        want = lib.segger_triplet_workspace_bytes(n)
        assert metric_fwd(lib, n=n, ws_bytes=want - 1) == EWORKSPACE, n
        assert err() == b"segger_metric_fwd: workspace %d < %d bytes" % (want - 1, want), n
    assert metric_fwd(lib, workspace=None) == EWORKSPACE and b"segger_metric_fwd: workspace" in err()
    assert metric_bwd(lib, grad_z=None) == EINVAL and b"segger_metric_bwd: grad_z is NULL" in err()


def test_edge_cos_argmax(lib):
    err = lib.segger_last_error
    assert lib.segger_edge_cos_argmax(None, None) == EINVAL and b"args is NULL" in err()
    for bad in (dict(n_rows=-1), dict(n_cols=-1), dict(n_edges=-1)):
        assert argmax(lib, **bad) == EINVAL and b"negative size" in err(), bad
    for bad in (dict(n_rows=0x7fffffff), dict(n_edges=0x7fffffff)):
        assert argmax(lib, **bad) == EINVAL and b"batch too large" in err(), bad
    assert argmax(lib, channels=0) == EINVAL and b"channels must be positive" in err()
    assert argmax(lib, indptr=None) == EINVAL and b"NULL graph array" in err()
    assert argmax(lib, col=None) == EINVAL and b"NULL graph array" in err()
    assert argmax(lib, z_src=None) == EINVAL and b"NULL embedding" in err()
    assert argmax(lib, z_dst=None) == EINVAL and b"NULL embedding" in err()
    for name in ("ld_zs", "ld_zd"):
        assert argmax(lib, **{name: CH - 1}) == EINVAL and b"ld < channels" in err(), name
    for name in ("max_sim", "max_eid", "seg_idx"):
        assert argmax(lib, **{name: None}) == EINVAL and b"NULL output" in err(), name
    assert argmax(lib, dtype=3) == EINVAL and b"segger_edge_cos_argmax: unknown dtype 3" in err()


def test_loss_combine(lib):
    err = lib.segger_last_error
    for name in ("segger_loss_combine_fwd", "segger_loss_combine_bwd"):
        word = name.encode() + b": 1..16 terms, no NULL pointer"
        call = getattr(lib, name)
        for n in (0, 17, -1):
            assert call(FAKE, FAKE, FAKE, n, FAKE, None) == EINVAL and word in err(), (name, n)
        for k in (0, 1, 2, 4):
            p = [FAKE, FAKE, FAKE, 3, FAKE]
            p[k] = None
            assert call(*p, None) == EINVAL and word in err(), (name, k)
    word = b"segger_loss_combine_partials_fwd: 1..16 terms, no NULL pointer"
    call = lib.segger_loss_combine_partials_fwd
    parts, counts, scales = (C.c_void_p * 3)(FAKE, FAKE, FAKE), (C.c_int64 * 3)(4, 0, 2), (C.c_float * 3)(1.0, 1.0, 1.0)
    host = [C.addressof(parts), C.addressof(counts), C.addressof(scales)]
    for n in (0, 17, -1):
        assert call(*host, FAKE, FAKE, n, FAKE, None) == EINVAL and word in err(), n
    for k in range(7):
        if k == 5:
            continue
        p = host + [FAKE, FAKE, 3, FAKE]
        p[k] = None
        assert call(*p, None) == EINVAL and word in err(), k
    counts[2] = -1
    assert call(*host, FAKE, FAKE, 3, FAKE, None) == EINVAL and b"segger_loss_combine_partials_fwd: bad term 2" in err()
    counts[2], parts[0] = 2, None
    assert call(*host, FAKE, FAKE, 3, FAKE, None) == EINVAL and b"segger_loss_combine_partials_fwd: bad term 0" in err()


def test_partial_count_and_workspace_bytes(lib):
    ns = (0, 1, 64, 65)
    assert [lib.segger_triplet_partial_count(n) for n in ns] == [0, 1, 1, 2]
    assert [lib.segger_triplet_workspace_bytes(n) for n in ns] == [20, 20, 20, 24]
    assert lib.segger_triplet_partial_count(-1) == 0 and lib.segger_triplet_workspace_bytes(-1) == 20
