"""Host layer of the forward projections (CPU): what the nine segger_linear_fwd* entry points and the two plane splitters
reject before they touch the device, with which code and which word in segger_last_error(), plus the literal tables of
segger_linear_supported and segger_linear_fwd_f32_split_supported.  Every pointer is a fake aligned address that is never
dereferenced, the stream is NULL and every call below fails a host check or has no rows: nothing is launched (no call
with rows and every argument valid, and in fp32 storage no pair whose FIRST side has rows and is valid).  No case depends
on the device's compute-unit count."""
import ctypes as C

import pytest

from segger_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2                          # include/segger_amd.h
F32, BF16, F16 = 0, 1, 2
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
N = 100                           # one 128-row block
DTYPES = (BF16, F16, F32)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def ld(given, width):
    return width if given is None else given


def fwd(lib, n=N, k=128, m=128, dtype=BF16, ldx=None, ldy=None, **p):
    a = dict(x=FAKE, w=FAKE, bias=FAKE, y=FAKE)
    a.update(p)
    return lib.segger_linear_fwd(a["x"], ld(ldx, k), a["w"], a["bias"], a["y"], ld(ldy, m), n, k, m, dtype, None)


def rowbias(lib, n=N, k=128, m=128, dtype=BF16, ldx=None, ldy=None, ld_rb=None, **p):
    a = dict(x=FAKE, w=FAKE, bias=FAKE, rowbias=FAKE, rowidx=FAKE, y=FAKE)
    a.update(p)
    return lib.segger_linear_fwd_rowbias(a["x"], ld(ldx, k), a["w"], a["bias"], a["rowbias"], ld(ld_rb, m), a["rowidx"], a["y"],
                                         ld(ldy, m), n, k, m, dtype, None)


def silu(lib, n=N, k=64, m=128, dtype=BF16, ldx=None, ldy=None, ld_gate=None, **p):
    a = dict(x=FAKE, w=FAKE, gate=FAKE, y=FAKE)
    a.update(p)
    return lib.segger_linear_fwd_silu_grad(a["x"], ld(ldx, k), a["w"], a["gate"], ld(ld_gate, m), a["y"], ld(ldy, m), n, k, m,
                                           dtype, None)


def split(lib, n=N, k=128, m=128, ldx=None, ldy=None, **p):
    a = dict(x=FAKE, w=FAKE, bias=FAKE, y=FAKE)
    a.update(p)
    return lib.segger_linear_fwd_f32_split(a["x"], ld(ldx, k), a["w"], a["bias"], a["y"], ld(ldy, m), n, k, m, None)


def split_rowbias(lib, n=N, k=128, m=128, ldx=None, ldy=None, ld_rb=None, **p):
    a = dict(x=FAKE, w=FAKE, rowbias=FAKE, rowidx=FAKE, y=FAKE)
    a.update(p)
    return lib.segger_linear_fwd_f32_split_rowbias(a["x"], ld(ldx, k), a["w"], a["rowbias"], ld(ld_rb, m), a["rowidx"], a["y"],
                                                   ld(ldy, m), n, k, m, None)


def act(lib, n=N, k=128, m=128, kind=1, ldx=None, ldy=None, ld_yact=None, **p):
    a = dict(x=FAKE, w=FAKE, bias=FAKE, y=FAKE, y_act=FAKE)
    a.update(p)
    return lib.segger_linear_fwd_f32_act(a["x"], ld(ldx, k), a["w"], a["bias"], a["y"], ld(ldy, m), a["y_act"], ld(ld_yact, m),
                                         kind, n, k, m, None)


def gate(lib, n=N, k=128, m=128, kind=1, planes=0, ldx=None, ldy=None, ld_gate=None, **p):
    a = dict(x=FAKE, w=FAKE, gate=FAKE, y=FAKE)
    a.update(p)
    return lib.segger_linear_fwd_f32_gate(a["x"], ld(ldx, k), a["w"], planes, a["gate"], ld(ld_gate, m), kind, a["y"], ld(ldy, m),
                                          n, k, m, None)


def side(k=128, m=128, n=N, **f):
    a = _lib.LinearArgs()
    a.x, a.ldx, a.w, a.bias, a.y, a.ldy, a.n_rows, a.m_out = FAKE, k, FAKE, FAKE, FAKE, m, n, m
    for name, v in f.items():
        setattr(a, name, v)
    return a


def ref(a):
    return None if a is None else C.byref(a)


def pair(lib, a, b, k=128, dtype=BF16):
    return lib.segger_linear_fwd_pair(ref(a), ref(b), k, dtype, None)


def pair_k(lib, a, ka, b, kb, dtype=BF16):
    return lib.segger_linear_fwd_pair_k(ref(a), ka, ref(b), kb, dtype, None)


# (call, fixed keywords, fp32 storage?, the pointers that must be given, the leading dimensions and the width they span)
SINGLE = [(fwd, dict(dtype=d), d == F32, ("x", "w", "y"), (("ldx", "k"), ("ldy", "m"))) for d in DTYPES] + [
    (rowbias, dict(dtype=d), d == F32, ("x", "w", "y"), (("ldx", "k"), ("ldy", "m"))) for d in DTYPES] + [
    (silu, dict(dtype=d), False, ("x", "w", "y", "gate"), (("ldx", "k"), ("ldy", "m"), ("ld_gate", "m"))) for d in (BF16, F16)] + [
    (split, {}, True, ("x", "w", "y"), (("ldx", "k"), ("ldy", "m"))),
    (split, dict(k=384), True, ("x", "w", "y"), (("ldx", "k"), ("ldy", "m"))),
    (split_rowbias, {}, True, ("x", "w", "y"), (("ldx", "k"), ("ldy", "m"))),
    (act, {}, True, ("x", "w", "y", "y_act"), (("ldx", "k"), ("ldy", "m"), ("ld_yact", "m"))),
    (act, dict(kind=2, k=64), True, ("x", "w", "y", "y_act"), (("ldx", "k"), ("ldy", "m"), ("ld_yact", "m"))),
    (gate, {}, True, ("x", "w", "y", "gate"), (("ldx", "k"), ("ldy", "m"), ("ld_gate", "m"))),
    (gate, dict(kind=2, planes=1), True, ("x", "w", "y", "gate"), (("ldx", "k"), ("ldy", "m"), ("ld_gate", "m"))),
    (gate, dict(planes=1, k=384), True, ("x", "w", "y", "gate"), (("ldx", "k"), ("ldy", "m"), ("ld_gate", "m")))]


def test_negative_row_count(lib):
    err = lib.segger_last_error
    for call, kw, _, _, _ in SINGLE:
        # ("bad sizes" / "negative size"; the two epilogue entries report it with their kind check, under their own name)
        word = b"segger_linear_fwd_f32_" + call.__name__.encode() if call in (act, gate) else b"size"
        assert call(lib, n=-1, **kw) == EINVAL and word in err(), (call.__name__, kw)


def test_zero_widths(lib):
    """m_out = 0 / k_in = 0: a bad size on the entries that take a dtype code, an unsupported shape on the fp32-only ones."""
    err = lib.segger_last_error
    for call, kw, _, _, _ in SINGLE:
        if "k" in kw:
            continue
        for bad in (dict(m=0), dict(k=0)):
            if call in (fwd, rowbias, silu):
                assert call(lib, **bad, **kw) == EINVAL and b"bad sizes" in err(), (call.__name__, kw, bad)
            else:
                assert call(lib, **bad, **kw) == EUNSUPPORTED and b"not supported" in err(), (call.__name__, kw, bad)
    for which in (0, 1):
        ab = [side(), side()]
        ab[which].m_out = 0
        assert pair(lib, *ab) == EINVAL and b"bad sizes" in err(), which
        ab = [side(), side()]
        ab[which].n_rows = -1
        assert pair(lib, *ab) == EINVAL and b"bad sizes" in err(), which
    assert pair(lib, side(n=-1), side(), dtype=F32) == EINVAL and b"bad sizes" in err()
    assert pair(lib, side(m=0), side(), dtype=F32) == EINVAL and b"bad sizes" in err()


def test_null_and_misaligned_pointers(lib):
    err = lib.segger_last_error
    for call, kw, f32, names, _ in SINGLE:
        for name in names:
            assert call(lib, **kw, **{name: None}) == EINVAL and b"NULL" in err(), (call.__name__, kw, name)
            assert call(lib, **kw, **{name: FAKE + 4}) == EINVAL and b"aligned" in err(), (call.__name__, kw, name)
        if f32 and call not in (split_rowbias, gate):          # the fp32 kernels read the bias 16 bytes at a time
            assert call(lib, **kw, bias=FAKE + 4) == EINVAL and b"aligned" in err(), (call.__name__, kw)


def test_leading_dimensions(lib):
    err = lib.segger_last_error
    sizes = dict(k=128, m=128)
    for call, kw, f32, _, lds in SINGLE:
        word = b"aligned" if f32 else b"leading dimension"
        step = 2 if f32 else 4              # 8 bytes past a 16-byte row; the 16-bit gate rows need 8 bytes only: 4 bytes past
        for name, width in lds:
            w = kw.get(width, 64 if (call is silu and width == "k") else sizes[width])
            assert call(lib, **kw, **{name: w - 1}) == EINVAL and word in err(), (call.__name__, kw, name)
            off = 2 if (call is silu and name == "ld_gate") else step
            assert call(lib, **kw, **{name: w + off}) == EINVAL and word in err(), (call.__name__, kw, name)


def test_unsupported_shapes_and_dtypes(lib):
    err = lib.segger_last_error
    for call, kw in ((fwd, dict(dtype=BF16)), (fwd, dict(dtype=F16)), (fwd, dict(dtype=F32)), (rowbias, dict(dtype=BF16)),
                     (rowbias, dict(dtype=F32)), (act, {}), (gate, {}), (split, {}), (split_rowbias, {}), (gate, dict(planes=1))):
        for bad in (dict(k=96), dict(m=96), dict(k=512)):
            assert call(lib, **bad, **kw) == EUNSUPPORTED and b"not supported" in err(), (call.__name__, kw, bad)
    for call in (fwd, rowbias):
        assert call(lib, dtype=3) == EUNSUPPORTED and b"not supported" in err(), call.__name__
    for call in (split, split_rowbias):                    # planes: 128 -> any multiple of 64, 384 -> 128 only
        assert call(lib, k=256) == EUNSUPPORTED and b"not supported" in err(), call.__name__
        assert call(lib, k=384, m=256) == EUNSUPPORTED and b"not supported" in err(), call.__name__
        assert call(lib, k=64) == EUNSUPPORTED and b"not supported" in err(), call.__name__


def test_row_bias(lib):
    err = lib.segger_last_error
    for dtype in DTYPES:
        step = 2 if dtype == F32 else 4
        assert rowbias(lib, dtype=dtype, rowidx=None) == EINVAL and b"together" in err(), dtype
        assert rowbias(lib, dtype=dtype, rowbias=None) == EINVAL and b"together" in err(), dtype
        assert rowbias(lib, dtype=dtype, rowbias=FAKE + 4) == EINVAL and b"table" in err(), dtype
        assert rowbias(lib, dtype=dtype, ld_rb=127) == EINVAL and b"table" in err(), dtype
        assert rowbias(lib, dtype=dtype, ld_rb=128 + step) == EINVAL and b"table" in err(), dtype
    for dtype in (BF16, F16):                              # the 16-bit row-bias kernel: k_in 64 and 128
        for k in (256, 384):
            assert rowbias(lib, dtype=dtype, k=k) == EUNSUPPORTED and b"segger_linear_fwd_rowbias" in err(), (dtype, k)
    assert rowbias(lib, dtype=F32, k=384) == EUNSUPPORTED and b"segger_linear_fwd_rowbias" in err()
    assert split_rowbias(lib, rowidx=None) == EINVAL and b"table" in err()
    assert split_rowbias(lib, rowbias=None) == EINVAL and b"table" in err()
    assert split_rowbias(lib, rowbias=None, rowidx=None) == EINVAL and b"table" in err()
    assert split_rowbias(lib, rowbias=FAKE + 4) == EINVAL and b"table" in err()
    assert split_rowbias(lib, ld_rb=127) == EINVAL and b"table" in err()
    assert split_rowbias(lib, ld_rb=130) == EINVAL and b"table" in err()


def test_epilogue_kinds(lib):
    err = lib.segger_last_error
    for kind in (0, 3, -1):
        assert act(lib, kind=kind) == EINVAL and b"act_kind" in err(), kind
        for planes in (0, 1):
            assert gate(lib, kind=kind, planes=planes) == EINVAL and b"gate_kind" in err(), (kind, planes)


def test_silu_grad_form(lib):
    err = lib.segger_last_error
    for bad in (dict(k=128), dict(k=256), dict(m=96), dict(dtype=F32), dict(dtype=3)):
        assert silu(lib, **bad) == EINVAL and b"k_in 64" in err(), bad


def test_the_fp32_epilogues_stop_at_k_256(lib):
    err = lib.segger_last_error
    for kind in (1, 2):
        assert act(lib, kind=kind, k=384) == EUNSUPPORTED and b"segger_linear_fwd_f32_act" in err(), kind
        assert gate(lib, kind=kind, k=384) == EUNSUPPORTED and b"segger_linear_fwd_f32_gate" in err(), kind
    assert rowbias(lib, dtype=F32, k=384, m=256) == EUNSUPPORTED and b"k_in" in err()
    assert gate(lib, planes=1, k=256) == EUNSUPPORTED and b"not supported" in err()        # planes: no such split kernel
    assert gate(lib, planes=1, k=384, m=256) == EUNSUPPORTED and b"not supported" in err()


def test_pair(lib):
    err = lib.segger_last_error
    assert pair(lib, None, side()) == EINVAL and b"NULL" in err()
    assert pair(lib, side(), None) == EINVAL and b"NULL" in err()
    assert pair_k(lib, None, 384, side(), 128) == EINVAL and b"NULL" in err()
    assert pair_k(lib, side(k=384), 384, None, 128) == EINVAL and b"NULL" in err()
    for ka, kb in ((128, 128), (384, 128), (256, 128)):    # one joint kernel, the instantiated mixed pair, two launches
        for dtype in (BF16, F16):
            for which in (0, 1):
                def call(**f):
                    ab = [side(k=ka), side(k=kb)]
                    for name, v in f.items():
                        setattr(ab[which], name, v)
                    return pair_k(lib, ab[0], ka, ab[1], kb, dtype)
                k = (ka, kb)[which]
                for name in ("x", "w", "y"):
                    assert call(**{name: None}) == EINVAL and b"NULL" in err(), (ka, kb, dtype, which, name)
                    assert call(**{name: FAKE + 4}) == EINVAL and b"aligned" in err(), (ka, kb, dtype, which, name)
                for f in (dict(ldx=k - 1), dict(ldx=k + 4), dict(ldy=127), dict(ldy=132)):
                    assert call(**f) == EINVAL and b"leading dimension" in err(), (ka, kb, dtype, which, f)
                assert call(m_out=96, ldy=96) == EUNSUPPORTED and b"not supported" in err(), (ka, kb, dtype, which)
    for which in (0, 1):
        ks = [128, 128]
        ks[which] = 96
        assert pair_k(lib, side(k=ks[0]), ks[0], side(k=ks[1]), ks[1]) == EUNSUPPORTED and b"not supported" in err(), which
    assert pair(lib, side(), side(), dtype=3) == EUNSUPPORTED and b"not supported" in err()
    # fp32 storage: two launches of the exact kernel, so only a bad FIRST side is refused before anything runs
    assert pair(lib, side(x=None), side(), dtype=F32) == EINVAL and b"NULL" in err()
    assert pair(lib, side(y=FAKE + 4), side(), dtype=F32) == EINVAL and b"aligned" in err()
    assert pair(lib, side(ldx=130), side(), dtype=F32) == EINVAL and b"aligned" in err()
    assert pair(lib, side(k=96), side(k=96), k=96, dtype=F32) == EUNSUPPORTED and b"not supported" in err()


def test_calls_without_rows_end_where_each_entry_always_ended_them(lib):
    """n_rows = 0: the entries of one operand set return SEGGER_OK right after their sizes and kinds, whatever else is
    wrong; the plane entries refuse an unsupported shape first; a 16-bit pair side is checked in full but for NULL."""
    err = lib.segger_last_error
    for call, kw in ((fwd, {}), (fwd, dict(dtype=F32)), (rowbias, {}), (rowbias, dict(dtype=F32)), (silu, {}), (act, {}), (gate, {}),
                     (gate, dict(planes=1))):
        for bad in (dict(k=96), dict(x=None), dict(y=FAKE + 4), dict(ldx=7)):
            assert call(lib, n=0, **kw, **bad) == 0, (call.__name__, kw, bad)
    assert silu(lib, n=0, dtype=F32) == 0 and act(lib, n=0, k=384) == 0 and gate(lib, n=0, k=384) == 0
    assert act(lib, n=0, kind=3) == EINVAL and gate(lib, n=0, kind=0) == EINVAL and fwd(lib, n=0, m=0) == EINVAL
    for call in (split, split_rowbias):
        for bad in (dict(k=256), dict(k=384, m=256), dict(m=96), dict(m=0)):
            assert call(lib, n=0, **bad) == EUNSUPPORTED and b"not supported" in err(), (call.__name__, bad)
        for bad in ({}, dict(x=None), dict(y=FAKE + 4), dict(ldx=7)):
            assert call(lib, n=0, **bad) == 0, (call.__name__, bad)
    assert split_rowbias(lib, n=0, rowbias=None, rowidx=None) == 0
    for which in (0, 1):
        def call(dtype=BF16, **f):
            ab = [side(), side()]
            ab[which].n_rows = 0
            for name, v in f.items():
                setattr(ab[which], name, v)
            return pair(lib, *ab, dtype=dtype)
        assert call(m_out=96) == EUNSUPPORTED and b"not supported" in err(), which
        assert call(dtype=3) == EUNSUPPORTED and b"not supported" in err(), which
        for name in ("x", "w", "y"):
            assert call(**{name: FAKE + 4}) == EINVAL and b"aligned" in err(), (which, name)
        for f in (dict(ldx=127), dict(ldx=132), dict(ldy=127), dict(ldy=132)):
            assert call(**f) == EINVAL and b"leading dimension" in err(), (which, f)
    assert pair_k(lib, side(n=0), 96, side(), 128) == EUNSUPPORTED and b"not supported" in err()
    # fp32 storage: as two segger_linear_fwd calls -- an empty first side passes whatever its shape, the second is refused
    assert pair_k(lib, side(n=0), 96, side(x=None), 128, dtype=F32) == EINVAL and b"NULL" in err()
    assert pair_k(lib, side(n=0, x=FAKE + 4), 128, side(k=96), 96, dtype=F32) == EUNSUPPORTED and b"not supported" in err()


def test_pair_width_of_zero(lib):
    """k_in <= 0 on the pair: an unsupported shape at 16 bit (only n_rows and m_out are sizes there), a bad size at fp32."""
    err = lib.segger_last_error
    for k in (0, -64):
        assert pair(lib, side(), side(), k=k) == EUNSUPPORTED and b"not supported" in err(), k
        assert pair_k(lib, side(), 128, side(), k) == EUNSUPPORTED and b"not supported" in err(), k
        assert pair_k(lib, side(), k, side(), 128) == EUNSUPPORTED and b"not supported" in err(), k
        assert pair(lib, side(), side(), k=k, dtype=F32) == EINVAL and b"bad sizes" in err(), k


def job(**f):
    j = _lib.PlanesJob()
    j.w, j.rows, j.cols, j.transpose, j.planes = FAKE, 128, 128, 0, FAKE
    for name, v in f.items():
        setattr(j, name, v)
    return j


def test_plane_splitters(lib):
    err = lib.segger_last_error
    planes = lib.segger_f32_split_planes
    assert planes(FAKE, -1, 128, 0, FAKE, None) == EINVAL and b"negative" in err()
    assert planes(FAKE, 128, -1, 0, FAKE, None) == EINVAL and b"negative" in err()
    assert planes(None, 128, 128, 0, FAKE, None) == EINVAL and b"NULL" in err()
    assert planes(FAKE, 128, 128, 0, None, None) == EINVAL and b"NULL" in err()
    assert planes(FAKE, 1 << 20, 1 << 20, 0, FAKE, None) == EINVAL and b"too large" in err()

    def many(jobs, n=None):
        arr = (_lib.PlanesJob * max(len(jobs), 1))(*jobs)
        return lib.segger_f32_split_planes_many(C.cast(arr, C.c_void_p), len(jobs) if n is None else n, None)
    assert many([job()], n=0) == EINVAL and b"jobs" in err()
    assert many([job()] * 33) == EINVAL and b"jobs" in err()
    assert lib.segger_f32_split_planes_many(None, 1, None) == EINVAL and b"jobs" in err()
    for which in (0, 1):
        for bad, word in ((dict(rows=-1), b"negative"), (dict(cols=-1), b"negative"), (dict(w=None), b"NULL"),
                          (dict(planes=None), b"NULL"), (dict(rows=1 << 20, cols=1 << 20), b"too large")):
            jobs = [job(), job()]
            jobs[which] = job(**bad)
            assert many(jobs) == EINVAL and word in err(), (which, bad)


def test_messages_carry_the_entry_points_own_name(lib):
    err = lib.segger_last_error
    fwd(lib, x=None)
    assert err().startswith(b"segger_linear_fwd: ")
    silu(lib, x=None)
    assert err().startswith(b"segger_linear_fwd_silu_grad: ")
    pair(lib, side(x=None), side())
    assert err().startswith(b"segger_linear_fwd_pair: ")
    pair_k(lib, side(k=384), 384, side(y=None), 128)
    assert err().startswith(b"segger_linear_fwd_pair: ")
    split(lib, x=None)
    assert err().startswith(b"segger_linear_fwd_f32_split: ")
    act(lib, x=None)
    assert err().startswith(b"segger_linear_fwd_f32_act: ")
    gate(lib, x=None)
    assert err().startswith(b"segger_linear_fwd_f32_gate: ")


def test_supported_tables(lib):
    ks, ms = (32, 64, 96, 128, 256, 384, 512), (0, 32, 64, 128, 192, 256, 384)
    grid = [(k, m, d) for k in ks for m in ms for d in (F32, BF16, F16)]
    ok = {(k, m, d) for k in (64, 128, 256, 384) for m in (64, 128, 192, 256, 384) for d in (F32, BF16, F16)}
    assert {c for c in grid if lib.segger_linear_supported(*c)} == ok
    assert not any(lib.segger_linear_supported(128, 128, d) for d in (-1, 3))
    split_ok = {(128, m) for m in (64, 128, 192, 256, 384)} | {(384, 128)}
    assert {(k, m) for k in ks for m in ms if lib.segger_linear_fwd_f32_split_supported(k, m)} == split_ok
