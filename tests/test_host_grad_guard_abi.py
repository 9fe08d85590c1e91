"""C-ABI surface of the gradient guard (CPU): the symbols exist with the documented signatures, the device struct has the
documented layout, the ABI version is still 32, every bad argument is rejected on the host with SEGGER_EINVAL and a message,
an empty table returns 0 without a device, and the workspace size is monotone in its arguments -- nothing is launched by any
call below (every pointer is a fake aligned address that is never dereferenced)."""
import ctypes as C
import math
import os
import re

import pytest

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def table(n=2, numel=5000, **bad):
    arr = (_lib.AdamTensor * max(n, 1))()
    for a in arr:
        a.param = a.grad = a.exp_avg = a.exp_avg_sq = a.step = FAKE
        a.numel = numel
    for k, v in bad.items():
        setattr(arr[0], k, v)
    return arr


def guard(lib, n=2, numel=5000, cfg="default", state=FAKE, workspace=FAKE, ws_bytes=1 << 20, tensors="default", **cfg_kw):
    c = _lib.GuardCfg(cfg_kw.get("max_norm", 1.0), cfg_kw.get("growth", 2.0), cfg_kw.get("backoff", 0.5),
                      cfg_kw.get("growth_interval", 2000), cfg_kw.get("flags", 0))
    cfg = C.byref(c) if cfg == "default" else cfg
    tensors = table(n, numel) if tensors == "default" else tensors
    return lib.segger_grad_guard(tensors, n, cfg, state, workspace, ws_bytes, None)


def guarded(lib, n=2, hyper=FAKE, state=FAKE, tensors="default"):
    return lib.segger_adam_step_guarded(table(n) if tensors == "default" else tensors, n, hyper, 0, None, 0, state, None)


def test_symbols_signatures_layout_and_abi_version(lib):
    want = {"segger_grad_guard_workspace_bytes": (C.c_int64, [i32, i64]),
            "segger_grad_guard": (C.c_int, [C.POINTER(_lib.AdamTensor), i32, C.POINTER(_lib.GuardCfg), vp, vp, i64, vp]),
            "segger_adam_step_guarded": (C.c_int, [C.POINTER(_lib.AdamTensor), i32, vp, i32, vp, i64, vp, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    S = _lib.GuardState
    assert C.sizeof(S) == 40 and C.sizeof(_lib.GuardCfg) == 32
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [
        ("coef", 0, 4), ("skip", 4, 4), ("norm", 8, 8), ("scale", 16, 4), ("growth_tracker", 20, 4), ("n_skipped", 24, 8),
        ("n_clipped", 32, 8)]
    from segger_amd import ops
    for name in ("GuardState", "grad_guard", "adam_step", "adam_init_state"):
        assert hasattr(ops, name)


def test_header_documents_the_struct_and_keeps_the_version():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segger_amd.h")).read()
    assert re.search(r"#define SEGGER_ABI_VERSION 32\b", header)
    body = re.search(r"typedef struct segger_guard_state \{(.*?)\} segger_guard_state;", header, re.S).group(1)
    assert re.findall(r"(\w+) (\w+);", body) == [("float", "coef"), ("int32_t", "skip"), ("double", "norm"), ("float", "scale"),
                                                  ("int32_t", "growth_tracker"), ("int64_t", "n_skipped"), ("int64_t", "n_clipped")]
    for word in ("clip_grad_norm_", "GradScaler", "segger_grad_guard_workspace_bytes", "segger_adam_step_guarded"):
        assert word in header, word


def test_grad_guard_rejections(lib):
    err = lib.segger_last_error
    # (every call below changes ONE argument of a call that would be accepted, and is refused before anything is launched)
    assert guard(lib, n=-1) == EINVAL and b"segger_grad_guard" in err()
    assert guard(lib, tensors=None) == EINVAL and b"NULL tensor table" in err()
    assert guard(lib, cfg=None) == EINVAL and b"cfg is NULL or misaligned" in err()
    assert guard(lib, cfg=C.cast(FAKE + 4, C.POINTER(_lib.GuardCfg))) == EINVAL and b"cfg is NULL or misaligned" in err()
    for state in (None, FAKE + 4):
        assert guard(lib, state=state) == EINVAL and b"state is NULL or misaligned" in err()
    for ws in (None, FAKE + 8, FAKE + 128):
        assert guard(lib, workspace=ws) == EINVAL and b"workspace is NULL or not 256-byte aligned" in err()
    need = lib.segger_grad_guard_workspace_bytes(2, 2 * 3)              # 5000 elements: 3 blocks a tensor
    assert need == 256 + 256
    assert guard(lib, ws_bytes=need - 1) == EINVAL and b"workspace" in err() and str(need).encode() in err()
    assert guard(lib, ws_bytes=0) == EINVAL and b"workspace" in err()
    assert guard(lib, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
    for bad in (-1.0, -0.0 - 1e-300, math.nan):
        assert guard(lib, max_norm=bad) == EINVAL and b"max_norm" in err(), bad
    for bad in (0.0, 1.0, 1.5, -0.5, math.nan):
        assert guard(lib, backoff=bad) == EINVAL and b"backoff" in err(), bad
    for bad in (0.999, 0.0, -2.0, math.nan, math.inf):
        assert guard(lib, growth=bad) == EINVAL and b"growth" in err(), bad
    assert guard(lib, growth_interval=-1) == EINVAL and b"growth_interval" in err()
    assert guard(lib, flags=2) == EINVAL and b"flags" in err()
    assert guard(lib, tensors=table(2, numel=-1)) == EINVAL and b"bad size" in err()
    assert guard(lib, tensors=table(2, step=None)) == EINVAL and b"NULL step" in err()
    assert guard(lib, tensors=table(2, grad=None)) == EINVAL and b"NULL pointer" in err()


def test_grad_guard_accepts_the_edges_of_the_configuration(lib):
    # an empty table launches nothing, and its configuration is still checked in full
    for ok in (dict(max_norm=0.0), dict(growth=1.0), dict(growth_interval=0), dict(backoff=1e-9), dict(flags=1)):
        assert guard(lib, n=0, tensors=None, state=None, workspace=None, ws_bytes=0, **ok) == 0, ok
    assert guard(lib, n=0, max_norm=-1.0) == EINVAL


def test_empty_table_returns_ok_without_a_device(lib):
    assert guard(lib, n=0, tensors=None, state=None, workspace=None, ws_bytes=0) == 0
    assert guard(lib, n=0) == 0
    assert lib.segger_adam_step_guarded(None, 0, FAKE, 0, None, 0, FAKE, None) == 0


def test_adam_step_guarded_rejections(lib):
    err = lib.segger_last_error
    for hyper in (None, FAKE + 4):
        assert guarded(lib, hyper=hyper) == EINVAL and b"segger_adam_step_guarded: hyper is NULL or misaligned" in err()
    for state in (None, FAKE + 4):
        assert guarded(lib, state=state) == EINVAL and b"segger_adam_step_guarded: state is NULL or misaligned" in err()
    assert guarded(lib, n=-1) == EINVAL and b"NULL tensor table" in err()
    assert guarded(lib, tensors=table(2, step=None)) == EINVAL and b"NULL step" in err()
    assert guarded(lib, tensors=table(2, exp_avg=None)) == EINVAL and b"NULL pointer" in err()


def test_workspace_size_is_monotone_and_what_the_header_says(lib):
    ws = lib.segger_grad_guard_workspace_bytes

    def up(x):
        return (x + 255) // 256 * 256
    last_n = -1
    for n in (0, 1, 31, 32, 33, 64, 65, 1000):
        last_b = -1
        for blocks in (0, 1, 15, 16, 17, 1000, 1 << 20, (1 << 31) - 2):
            got = ws(n, blocks)
            assert got == up(16 * blocks) + up(8 * n), (n, blocks)
            assert got >= last_b and got >= ws(max(n - 1, 0), blocks)
            last_b = got
        assert ws(n, 0) >= last_n
        last_n = ws(n, 0)
    for bad in ((-1, 0), (0, -1), (1, 1 << 40)):
        assert ws(*bad) == EINVAL and b"segger_grad_guard_workspace_bytes" in lib.segger_last_error(), bad
