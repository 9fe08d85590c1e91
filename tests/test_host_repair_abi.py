"""The C-ABI surface of segger_rings_resort and the refusals of segger_amd.repair's wrappers, without a GPU: the symbol
and its signature, ABI version 32 (purely additive), every rejection on fake pointers that are never dereferenced --
answered with an error code and a message, nothing launched --, and what the Python side raises before the device is asked."""
import ctypes as C

import pytest
import torch

import repair_cases as rc
import simplify_cases as sc
from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def resort(lib, P=3, V=20, small=256, ws_bytes=1 << 20, **p):
    a = dict(ring_offsets=FAKE, xy=FAKE, select=FAKE, xy_out=FAKE + 4096, vertex_index=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_rings_resort(a["ring_offsets"], a["xy"], P, V, a["select"], a["xy_out"], a["vertex_index"], small, a["workspace"],
                                   ws_bytes, None)


def test_symbol_signature_and_abi_version(lib):
    sig = (C.c_int, [vp, vp, i64, i64, vp, vp, vp, i32, vp, i64, vp])
    assert hasattr(lib, "segger_rings_resort") and _lib.EXPORTS["segger_rings_resort"] == sig
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION         # purely additive
    import segger_amd
    from segger_amd import repair
    assert segger_amd.resort_rings is repair.resort_rings and segger_amd.repair_rings is repair.repair_rings
    assert repair.COUNTER_NAMES == rc.COUNTERS
    assert (repair.STATUS_VALID, repair.STATUS_REPAIRED, repair.STATUS_INVALID) == (0, 1, 2)


def test_rejections(lib):
    err = lib.segger_last_error
    assert resort(lib, P=-1) == EINVAL and b"negative" in err()
    assert resort(lib, V=-1) == EINVAL and b"negative" in err()
    assert resort(lib, P=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert resort(lib, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
    for s in (-1, 257):
        assert resort(lib, small=s) == EINVAL and b"small_max_verts" in err()
    for name in ("ring_offsets", "workspace", "xy_out", "vertex_index"):
        assert resort(lib, **{name: None}) == EINVAL and b"NULL pointer" in err(), name
    assert resort(lib, xy=None) == EINVAL and b"NULL xy" in err()
    for name in ("ring_offsets", "vertex_index"):
        assert resort(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("xy", "xy_out"):
        assert resort(lib, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), name
    assert resort(lib, workspace=FAKE + 64) == EINVAL and b"256-byte aligned" in err()
    assert resort(lib, xy_out=FAKE) == EINVAL and b"xy_out must not be xy" in err()
    need = 256 + 2 * 256                                             # the words and two lists of three int32
    assert resort(lib, ws_bytes=need - 1) == EINVAL and str(need).encode() in err()
    assert lib.segger_simplify_rings_workspace_bytes(3, 0) >= need   # what the Python side passes is enough
    for P in (1, 1000, 1 << 20):
        assert lib.segger_simplify_rings_workspace_bytes(P, 0) >= 256 + 2 * ((4 * P + 255) // 256 * 256)


def test_empty_input_returns_ok_without_a_device(lib):
    assert resort(lib, P=0, V=0, ws_bytes=0, ring_offsets=None, xy=None, select=None, xy_out=None, vertex_index=None, workspace=None) == 0


def test_python_side_refusals():
    from segger_amd import repair_rings, resort_rings
    off, xy = (torch.from_numpy(t) for t in sc.csr([rc.SPECIAL["bow_tie"], rc.SPECIAL["collinear"]]))
    for bad in ("abort", None, 0, "RAISE"):
        with pytest.raises(ValueError, match="on_failure"):
            repair_rings(off, xy, on_failure=bad)
    for bad in (torch.ones(3, dtype=torch.bool), torch.ones(2, 1, dtype=torch.bool), torch.ones(2), torch.ones(2, dtype=torch.int64),
                [True, False]):
        with pytest.raises(ValueError, match="select"):
            resort_rings(off, xy, bad)
    for bad in ("small", 0, "LARGE"):
        with pytest.raises(ValueError, match="_route"):
            resort_rings(off, xy, _route=bad)
    for fn in (resort_rings, repair_rings):
        with pytest.raises(ValueError, match="ring_offsets"):
            fn(off.float(), xy)
        with pytest.raises(ValueError, match="xy"):
            fn(off, xy[:, :1])
        with pytest.raises(ValueError, match="tensors"):
            fn(off.numpy(), xy)
    long_off, long_xy = (torch.from_numpy(t) for t in sc.csr([rc.SPECIAL["bow_tie"], sc.star_ring(rc.MAX_VERTS + 1, 5)]))
    for fn in (resort_rings, repair_rings):
        with pytest.raises(ValueError, match="polygon 1 has 4097 vertices"):    # n = 4097 is refused, and named
            fn(long_off, long_xy)
    for fn in (lambda: resort_rings(off, xy), lambda: resort_rings(off, xy, torch.tensor([True, False])), lambda: repair_rings(off, xy),
               lambda: repair_rings(off, xy, on_failure="drop")):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only.*repair_cases"):   # no CPU fallback; the oracle is named
            fn()
