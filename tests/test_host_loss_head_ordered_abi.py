"""C-ABI surface of the ordered loss head (CPU): the three symbols exist with the documented signatures, the argument struct
and the ABI version are what they were (no layout changed), bad arguments are rejected on the host, and the workspace
query is monotone in each of its inputs and never below the plain head's -- nothing is launched by any call below (every
pointer is a fake aligned address that is never dereferenced)."""
import ctypes as C

import pytest

from segger_amd import _lib

EINVAL = -1
FAKE = 0x10000                    # a non-NULL, 256-byte aligned address
i64 = C.c_int64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def args(**kw):
    a = _lib.LossHeadArgs()
    for f in ("z_tx", "z_bd", "tx_pos", "tx_neg", "bd_pos", "bd_neg", "bd_dpos", "bd_dneg", "bd_w", "sg_src", "sg_pos", "sg_neg",
              "sg_pos_indptr", "sg_pos_eid", "a", "b", "out", "grad_raw", "tx_w", "grad_tx", "grad_bd", "workspace"):
        setattr(a, f, FAKE)
    a.n_tx, a.n_bd, a.n_sg, a.channels, a.dtype = 100, 10, 50, 64, 0
    a.ld_ztx = a.ld_zbd = a.ld_gtx = 64
    a.workspace_bytes = 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_signatures_and_an_unchanged_layout(lib):
    want = {"segger_loss_head_ordered_workspace_bytes": (C.c_size_t, [i64, i64, i64]),
            "segger_loss_head_ordered_fwd": (C.c_int, [C.POINTER(_lib.LossHeadArgs), C.c_void_p]),
            "segger_loss_head_ordered_bwd": (C.c_int, [C.POINTER(_lib.LossHeadArgs), C.c_void_p])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == _lib.ABI_VERSION == 32
    assert C.sizeof(_lib.LossHeadArgs) == 344 and _lib.LossHeadArgs.reserved_.offset == 292
    from segger_amd import ops
    import inspect
    assert inspect.signature(ops.LossHeadSpec.__init__).parameters["deterministic"].default is False


def test_rejections_before_any_launch(lib):
    err = lib.segger_last_error
    for fn in (lib.segger_loss_head_ordered_fwd, lib.segger_loss_head_ordered_bwd):
        who = b"segger_loss_head_ordered_"
        assert fn(None, None) == EINVAL and who in err()
        assert fn(C.byref(args(channels=48)), None) == EINVAL and b"channels" in err()
        assert fn(C.byref(args(dtype=7)), None) == EINVAL and b"dtype" in err()
        assert fn(C.byref(args(n_tx=-1)), None) == EINVAL and b"negative" in err()
        assert fn(C.byref(args(n_tx=1 << 29)), None) == EINVAL and b"too large" in err()
        for chain in ("tx_state", "tx_next", "tx_hot_id", "tx_hot_acc"):
            assert fn(C.byref(args(**{chain: FAKE})), None) == EINVAL and b"keeps no chains" in err(), chain
        assert fn(C.byref(args(workspace=FAKE + 64)), None) == EINVAL and b"256-byte aligned" in err()
        need = lib.segger_loss_head_ordered_workspace_bytes(100, 10, 50)
        assert fn(C.byref(args(workspace_bytes=need - 1)), None) != 0 and str(need).encode() in err()
        assert fn(C.byref(args(reserved_=_lib.LOSS_HEAD_DEFER_FINISH)), None) == EINVAL and b"DEFER_FINISH needs grad_out" in err()
    bwd = lib.segger_loss_head_ordered_bwd
    assert bwd(C.byref(args(tx_w=None)), None) == EINVAL and b"tx_w" in err()
    assert bwd(C.byref(args(grad_tx=None)), None) == EINVAL and b"grad_tx" in err()
    assert bwd(C.byref(args(grad_bd=None)), None) == EINVAL and b"grad_bd" in err()
    assert bwd(C.byref(args(sg_pos_indptr=None)), None) == EINVAL and b"grouping by positive row" in err()


def test_workspace_grows_with_every_input_and_holds_the_plain_one(lib):
    ws, plain = lib.segger_loss_head_ordered_workspace_bytes, lib.segger_loss_head_workspace_bytes
    sizes = (0, 1, 63, 64, 65, 1000, 44000, 1 << 20)
    for k in range(3):
        for others in ((0, 0), (7, 300), (5000, 40000)):
            last = -1
            for n in sizes:
                shape = list(others)
                shape.insert(k, n)
                got = ws(*shape)
                assert got >= last and got % 256 == 0, (k, shape)
                # the partial sums of the plain head, two key arrays, the segment offsets
                n_tx, n_bd, n_sg = shape
                assert got >= plain(*shape) + 2 * 8 * (2 * n_tx + 2 * n_bd + n_sg) + 4 * (n_tx + n_bd + 1)
                last = got
    assert ws(-5, -5, -5) == ws(0, 0, 0) > 0
