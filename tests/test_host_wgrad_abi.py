"""Host layer of the weight-gradient entry points (CPU): what segger_linear_wgrad, _dx, _pair, _f32_split and
segger_posmlp_wgrad reject before they touch the device, with which code and which words in segger_last_error(), plus the
literal tables of the *_supported queries and of segger_linear_wgrad_workspace_bytes.  Every pointer is a fake aligned
address that is never dereferenced, the stream is NULL and every call below fails a host check: nothing is launched and
nothing is zeroed (no n_rows = 0 call, no call with every argument valid)."""
import ctypes as C

import pytest

from segger_amd import _lib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -4          # include/segger_amd.h
F32, BF16, F16 = 0, 1, 2
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
N = 100                           # 7 stages of 16 rows: one workgroup
BIG = 1 << 40                     # workspace_bytes that is never short


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def need(lib, m, k, n=N):
    return lib.segger_linear_wgrad_workspace_bytes(n, m, k)


def plain(lib, n=N, m=384, k=128, dtype=BF16, ws_bytes=BIG, ld_dy=None, ld_x=None, **p):
    a = dict(dy=FAKE, x=FAKE, grad_w=FAKE, grad_b=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_linear_wgrad(a["dy"], m if ld_dy is None else ld_dy, a["x"], k if ld_x is None else ld_x, n, m, k, dtype,
                                   a["grad_w"], a["grad_b"], a["workspace"], ws_bytes, None)


def with_dx(lib, n=N, m=384, k=128, dtype=BF16, ws_bytes=BIG, ld_dy=None, ld_x=None, ld_dx=None, ld_gate=0, **p):
    a = dict(dy=FAKE, x=FAKE, w_t=FAKE, grad_w=FAKE, grad_b=FAKE, dx=FAKE, gate=None, workspace=FAKE)
    a.update(p)
    return lib.segger_linear_wgrad_dx(a["dy"], m if ld_dy is None else ld_dy, a["x"], k if ld_x is None else ld_x, a["w_t"], n,
                                      m, k, dtype, a["grad_w"], a["grad_b"], a["dx"], k if ld_dx is None else ld_dx,
                                      a["gate"], ld_gate, a["workspace"], ws_bytes, None)


def split(lib, n=N, m=384, k=128, ws_bytes=BIG, ld_dy=None, ld_x=None, **p):
    a = dict(dy=FAKE, x=FAKE, grad_w=FAKE, grad_b=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_linear_wgrad_f32_split(a["dy"], m if ld_dy is None else ld_dy, a["x"], k if ld_x is None else ld_x, n, m,
                                             k, a["grad_w"], a["grad_b"], a["workspace"], ws_bytes, None)


def posmlp(lib, n=N, dtype=BF16, ws_bytes=BIG, ld=64, **p):
    a = dict(dz1=FAKE, pn=FAKE, grad_w0=FAKE, grad_b0=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_posmlp_wgrad(a["dz1"], ld, a["pn"], n, 10000.0, dtype, a["grad_w0"], a["grad_b0"], a["workspace"],
                                   ws_bytes, None)


def side(m, k=128, dx=False, n=N, **f):
    a = _lib.WgradArgs()
    a.dy, a.ld_dy, a.x, a.ld_x, a.n_rows, a.m_out = FAKE, m, FAKE, k, n, m
    a.grad_w, a.grad_b, a.workspace, a.workspace_bytes = FAKE, FAKE, FAKE, BIG
    if dx:
        a.w_t, a.dx, a.ld_dx = FAKE, FAKE, k
    for name, v in f.items():
        setattr(a, name, v)
    return a


def pair(lib, a, b, k=128, dtype=BF16):
    return lib.segger_linear_wgrad_pair(None if a is None else C.byref(a), None if b is None else C.byref(b), k, dtype, None)


def test_bad_sizes_and_null_grad_w(lib):
    err = lib.segger_last_error
    for call in (plain, with_dx):
        for bad in (dict(n=-1), dict(m=0), dict(k=0)):
            assert call(lib, **bad) == EINVAL and b"bad sizes" in err(), (call.__name__, bad)
        assert call(lib, grad_w=None) == EINVAL and b"grad_w" in err(), call.__name__
    assert split(lib, n=-1) == EINVAL and b"bad sizes" in err()
    assert split(lib, grad_w=None) == EINVAL and b"grad_w" in err()
    assert posmlp(lib, n=-1) == EINVAL and b"negative" in err()
    assert posmlp(lib, grad_w0=None) == EINVAL and b"grad_w" in err()
    assert posmlp(lib, dtype=F32) == EINVAL and b"bf16 / f16 only" in err()
    assert pair(lib, side(384, grad_w=None), side(128)) == EINVAL and b"grad_w" in err()
    assert pair(lib, side(384), side(128, grad_w=None)) == EINVAL and b"grad_w" in err()


def test_null_and_misaligned_inputs(lib):
    err = lib.segger_last_error
    cases = [(plain, {}, ("dy", "x")), (plain, dict(dtype=F16), ("dy", "x")), (plain, dict(dtype=F32), ("dy", "x")),
             (with_dx, {}, ("dy", "x", "w_t", "dx")), (posmlp, {}, ("dz1", "pn"))]
    for call, kw, names in cases:
        for name in names:
            assert call(lib, **kw, **{name: None}) == EINVAL and b"NULL" in err(), (call.__name__, kw, name)
            assert call(lib, **kw, **{name: FAKE + 4}) == EINVAL and b"aligned" in err(), (call.__name__, kw, name)
    for name in ("dy", "x"):
        assert split(lib, **{name: None}) == EINVAL and b"16-byte aligned" in err(), name
        assert split(lib, **{name: FAKE + 4}) == EINVAL and b"16-byte aligned" in err(), name
    for dx, names in ((False, ("dy", "x")), (True, ("dy", "x", "dx"))):
        for name in names:
            for which in (0, 1):
                ab = [side(384, dx=dx), side(128, dx=dx)]
                setattr(ab[which], name, None)
                assert pair(lib, *ab) == EINVAL and b"NULL" in err(), (dx, name, which)
                setattr(ab[which], name, FAKE + 4)
                assert pair(lib, *ab) == EINVAL and b"aligned" in err(), (dx, name, which)
    ab = [side(384, dx=True), side(128, dx=True, w_t=FAKE + 4)]
    assert pair(lib, *ab) == EINVAL and b"aligned" in err()
    assert pair(lib, None, side(128)) == EINVAL and b"NULL" in err()
    assert pair(lib, side(384), None) == EINVAL and b"NULL" in err()


def test_leading_dimensions(lib):
    err = lib.segger_last_error
    m, k = 384, 128
    for call, kw in ((plain, {}), (plain, dict(dtype=F32)), (with_dx, {}), (split, {})):
        word = b"16-byte aligned" if call is split else b"leading dimension"
        assert call(lib, **kw, ld_dy=m - 1) == EINVAL and word in err(), (call.__name__, kw)
        assert call(lib, **kw, ld_x=k - 1) == EINVAL and word in err(), (call.__name__, kw)
    assert with_dx(lib, ld_dx=k - 1) == EINVAL and b"leading dimension" in err()
    for call in (plain, with_dx):                      # 16-bit rows must start on 16 bytes: 8 elements
        assert call(lib, ld_dy=m + 4) == EINVAL and b"leading dimension" in err(), call.__name__
        assert call(lib, ld_x=k + 4) == EINVAL and b"leading dimension" in err(), call.__name__
    assert with_dx(lib, ld_dx=k + 4) == EINVAL and b"leading dimension" in err()
    assert split(lib, ld_dy=m + 2) == EINVAL and b"16-byte aligned" in err()        # fp32 rows: 4 elements
    assert split(lib, ld_x=k + 2) == EINVAL and b"16-byte aligned" in err()
    assert posmlp(lib, ld=63) == EINVAL and b"aligned" in err()
    assert posmlp(lib, ld=68) == EINVAL and b"aligned" in err()
    for dx in (False, True):
        for f in (dict(ld_dy=127), dict(ld_dy=132), dict(ld_x=k - 1), dict(ld_x=k + 4)) + ((dict(ld_dx=k - 1), dict(ld_dx=k + 4)) if dx else ()):
            assert pair(lib, side(384, dx=dx), side(128, dx=dx, **f)) == EINVAL and b"leading dimension" in err(), (dx, f)


def test_gate_form(lib):
    err = lib.segger_last_error
    assert with_dx(lib, m=192, gate=FAKE, ld_gate=128) == EINVAL and b"gate form" in err()
    assert with_dx(lib, m=64, gate=FAKE, ld_gate=128) == EINVAL and b"gate form" in err()
    for m in (384, 128):
        assert with_dx(lib, m=m, gate=FAKE + 4, ld_gate=128) == EINVAL and b"gate" in err() and b"aligned" in err()
        assert with_dx(lib, m=m, gate=FAKE, ld_gate=127) == EINVAL and b"gate" in err()
        assert with_dx(lib, m=m, gate=FAKE, ld_gate=132) == EINVAL and b"gate" in err()


def test_unsupported_shapes_and_dtypes(lib):
    err = lib.segger_last_error
    for call, kw in ((plain, {}), (plain, dict(dtype=F16)), (plain, dict(dtype=F32)), (with_dx, {}), (split, {})):
        assert call(lib, m=192, k=96, **kw) == EUNSUPPORTED and b"not supported" in err(), (call.__name__, kw)
    assert plain(lib, dtype=3) == EUNSUPPORTED and b"not supported" in err()
    assert with_dx(lib, k=256) == EUNSUPPORTED and b"not supported" in err()
    assert with_dx(lib, dtype=F32) == EUNSUPPORTED and b"not supported" in err()
    assert split(lib, m=0) == EUNSUPPORTED and b"not supported" in err()
    for dx in (False, True):                           # both sides go to their own entry point, which refuses
        assert pair(lib, side(192, k=96, dx=dx), side(192, k=96, dx=dx), k=96) == EUNSUPPORTED and b"not supported" in err()


def test_workspace(lib):
    err = lib.segger_last_error
    for call, m, k in ((plain, 384, 128), (plain, 192, 64), (with_dx, 384, 128), (with_dx, 64, 128), (split, 384, 128)):
        kw = dict(m=m, k=k)
        assert call(lib, ws_bytes=need(lib, m, k) - 1, **kw) == EWORKSPACE and b"workspace" in err(), (call.__name__, m, k)
        assert str(need(lib, m, k)).encode() in err()
        assert call(lib, workspace=None, **kw) == EWORKSPACE and b"workspace" in err(), (call.__name__, m, k)
    assert plain(lib, dtype=F32, ws_bytes=need(lib, 384, 128) - 1) == EWORKSPACE and b"workspace" in err()
    assert posmlp(lib, ws_bytes=need(lib, 64, 256) - 1) == EWORKSPACE and b"workspace" in err()
    assert posmlp(lib, workspace=None) == EWORKSPACE and b"workspace" in err()
    # the pair: a shape with a paired kernel (384 / 128), one that goes to two launches (192 / 64: side a is short, so
    # nothing is launched before the refusal), each with and without the data gradient
    for ma, mb in ((384, 128), (192, 64)):
        for dx in (False, True):
            for which in (0, 1) if ma == 384 else (0,):
                ab = [side(ma, dx=dx), side(mb, dx=dx)]
                ab[which].workspace_bytes = need(lib, (ma, mb)[which], 128) - 1
                assert pair(lib, *ab) == EWORKSPACE and b"workspace" in err(), (ma, mb, dx, which)
                ab[which].workspace_bytes, ab[which].workspace = BIG, None
                assert pair(lib, *ab) == EWORKSPACE and b"workspace" in err(), (ma, mb, dx, which)
    assert pair(lib, side(384, workspace_bytes=need(lib, 384, 128) - 1), side(128), dtype=F32) == EWORKSPACE    # fp32: two launches


def test_posmlp_bwd_workspace(lib):
    err = lib.segger_last_error
    want = lib.segger_posmlp_bwd_pair_workspace_bytes(N, N)
    assert (lib.segger_posmlp_bwd_pair_workspace_bytes(N, 0), want) == (2720256, 2802688)
    assert lib.segger_posmlp_bwd_workspace_bytes(N) == 2720256 and lib.segger_posmlp_bwd_pair_workspace_bytes(0, 0) == 16

    def bwd(ws, ws_bytes):
        return lib.segger_posmlp_bwd_pair(FAKE, 64, FAKE, FAKE, N, FAKE, 64, FAKE, FAKE, N, FAKE, 10000.0, BF16, FAKE, FAKE,
                                          FAKE, FAKE, ws, ws_bytes, None)
    assert bwd(FAKE, want - 1) == EWORKSPACE and b"workspace" in err() and str(want).encode() in err()
    assert bwd(None, BIG) == EWORKSPACE and b"workspace" in err()


def test_a_workgroups_slab_stays_under_1_gib(lib):
    """100 rows = 7 stages on one workgroup: its slab spans 7 * 16 rows of ld elements of 2 bytes, and the buffer
    resource's out-of-range offset is 2^30: ld = 4793496 is the first multiple of 8 with 224 * ld >= 2^30."""
    err = lib.segger_last_error
    ld = 4793496
    assert 224 * ld >= 1 << 30 > 224 * (ld - 8)
    assert plain(lib, ld_dy=ld) == EINVAL and b"1 GiB" in err()
    assert plain(lib, ld_x=ld) == EINVAL and b"1 GiB" in err()
    assert with_dx(lib, ld_dy=ld) == EINVAL and b"1 GiB" in err()
    assert with_dx(lib, ld_x=ld) == EINVAL and b"1 GiB" in err()
    assert with_dx(lib, gate=FAKE, ld_gate=ld) == EINVAL and b"1 GiB" in err()
    assert posmlp(lib, ld=ld) == EINVAL and b"1 GiB" in err()
    for dx in (False, True):
        assert pair(lib, side(384, dx=dx), side(128, dx=dx, ld_dy=ld)) == EINVAL and b"1 GiB" in err()
        assert pair(lib, side(384, dx=dx, ld_x=ld), side(128, dx=dx)) == EINVAL and b"1 GiB" in err()


def test_messages_carry_the_entry_points_own_name(lib):
    err = lib.segger_last_error
    plain(lib, n=-1)
    assert err().startswith(b"segger_linear_wgrad: ")
    with_dx(lib, dy=None)
    assert err().startswith(b"segger_linear_wgrad_dx: ")
    split(lib, workspace=None)
    assert err().startswith(b"segger_linear_wgrad_f32_split: ")
    posmlp(lib, pn=None)
    assert err().startswith(b"segger_posmlp_wgrad: ")
    pair(lib, side(384, dy=None), side(128))
    assert err().startswith(b"segger_linear_wgrad_pair: ")
    pair(lib, side(192, dy=None), side(64))            # (no paired kernel for 192 / 64: still the pair's own check)
    assert err().startswith(b"segger_linear_wgrad_pair: ")


def test_supported_tables(lib):
    ms, ks = (64, 96, 128, 192, 384), (64, 96, 128, 256)
    grid = [(m, k, d) for m in ms for k in ks for d in (F32, BF16, F16)]
    plain_ok = {(m, k, d) for m in (64, 128, 192, 384) for k in (64, 128, 256) for d in (F32, BF16, F16)}
    dx_ok = {(m, 128, d) for m in (64, 128, 192, 384) for d in (BF16, F16)}
    gate_ok = {(m, 128, d) for m in (128, 384) for d in (BF16, F16)}
    for name, ok in (("segger_linear_wgrad_supported", plain_ok), ("segger_linear_wgrad_dx_supported", dx_ok),
                     ("segger_linear_wgrad_dx_gate_supported", gate_ok)):
        assert {c for c in grid if getattr(lib, name)(*c)} == ok, name
    split_ok = {(384, 128), (128, 128), (128, 256), (64, 256)}
    assert {(m, k) for m in ms for k in ks if lib.segger_linear_wgrad_f32_split_supported(m, k)} == split_ok


def test_workspace_bytes(lib):
    ns = (0, 1, 16, 17, 8192, 10 ** 6)
    want = {(384, 128): [16, 6538752, 6538752, 6538752, 9510912, 57065472],
            (64, 256): [16, 2171136, 2171136, 2171136, 3158016, 52633600],
            (192, 64): [16, 1647360, 1647360, 1647360, 2396160, 39936000]}
    for (m, k), sizes in want.items():
        assert [lib.segger_linear_wgrad_workspace_bytes(n, m, k) for n in ns] == sizes, (m, k)
    assert lib.segger_linear_wgrad_workspace_bytes(N, 192, 96) == 16 == lib.segger_linear_wgrad_workspace_bytes(-1, 384, 128)
