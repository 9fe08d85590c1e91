"""C-ABI surface of the morphology entry points (CPU): the symbols exist with the documented signatures, the workspace
size is what the header says, the ABI version is still 32, bad arguments are rejected on the host with SEGGER_EINVAL and
a message, and an empty input returns 0 without a device -- nothing is launched by any call below (every pointer is a
fake aligned address that is never dereferenced).  A ring above SEGGER_MORPH_MAX_VERTS is refused by the Python wrapper
before the call, as include/segger_amd.h says: the ring lengths are device memory to the C entry point."""
import ctypes as C

import pytest
import torch

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i64 = C.c_void_p, C.c_int64
PTRS = ("ring_offsets", "xy", "props", "workspace")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def props(lib, P=10, V=50, ws_bytes=1 << 20, **p):
    a = {name: FAKE for name in PTRS}
    a.update(p)
    return lib.segger_polygon_props(a["ring_offsets"], a["xy"], P, V, a["props"], a["workspace"], ws_bytes, None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_morphology_workspace_bytes": (C.c_int64, [i64]),
            "segger_polygon_props": (C.c_int, [vp, vp, i64, i64, vp, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION
    assert (_lib.MORPH_MAX_VERTS, _lib.MORPH_COLS) == (4096, 12)
    import segger_amd
    from segger_amd import morphology
    assert segger_amd.morphology is morphology
    for name in ("polygon_props", "morphology_features", "rings_from_padded"):
        assert getattr(segger_amd, name) is getattr(morphology, name)


def test_workspace_size_is_what_the_header_says(lib):
    def up(x):
        return (x + 255) // 256 * 256
    for P in (0, 1, 63, 64, 65, 1000, 10 ** 6, (1 << 31) - 2):
        assert lib.segger_morphology_workspace_bytes(P) == 256 + 2 * up(4 * P), P
    for P in (-1, (1 << 31) - 1):
        assert lib.segger_morphology_workspace_bytes(P) == EINVAL and b"n_polygons" in lib.segger_last_error(), P


def test_polygon_props_rejections(lib):
    err = lib.segger_last_error
    assert props(lib, P=-1) == EINVAL and b"negative" in err()
    assert props(lib, V=-1) == EINVAL and b"negative" in err()
    assert props(lib, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
    assert props(lib, P=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    for name in PTRS:
        assert props(lib, **{name: None}) == EINVAL and b"NULL" in err(), name
        assert props(lib, **{name: FAKE + 4}) == EINVAL and b"aligned" in err(), name
    assert props(lib, xy=FAKE + 8) == EINVAL and b"16-byte aligned" in err()
    need = lib.segger_morphology_workspace_bytes(10)
    assert props(lib, ws_bytes=need - 1) == EINVAL and b"workspace" in err() and str(need).encode() in err()
    assert props(lib, ws_bytes=0) == EINVAL and b"workspace" in err()


def test_no_polygons_return_ok_without_a_device(lib):
    assert props(lib, P=0, V=0, ws_bytes=0, ring_offsets=None, xy=None, props=None, workspace=None) == 0
    assert props(lib, P=0) == 0


def test_python_side_refuses_the_cap_bad_arguments_and_cpu_tensors():
    from segger_amd import morphology as mo
    cap = _lib.MORPH_MAX_VERTS
    ring = torch.rand(cap + 1, 2, dtype=torch.float64)
    offsets = torch.tensor([0, 3, 3 + cap + 1], dtype=torch.int64)
    with pytest.raises(ValueError, match=rf"polygon 1 has {cap + 1} vertices.*SEGGER_MORPH_MAX_VERTS = {cap}"):
        mo.polygon_props(offsets, torch.cat([torch.rand(3, 2, dtype=torch.float64), ring]))
    closed = torch.cat([ring[:cap], ring[:1]])                       # cap vertices and a closing duplicate: within the cap
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        mo.polygon_props(torch.tensor([0, cap + 1]), closed)
    with pytest.raises(ValueError, match=r"polygon 0 has"):
        mo.polygon_props(torch.tensor([0, cap + 2]), torch.cat([closed, ring[:1]]))
    with pytest.raises(ValueError, match="ring_offsets"):
        mo.polygon_props(torch.zeros(3, dtype=torch.float32), torch.zeros(4, 2))
    with pytest.raises(ValueError, match="ring_offsets"):
        mo.polygon_props(torch.zeros(0, dtype=torch.int64), torch.zeros(4, 2))
    for xy in (torch.zeros(4, 3), torch.zeros(8), torch.zeros(4, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="xy"):
            mo.polygon_props(torch.tensor([0, 4]), xy)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        mo.morphology_features(torch.tensor([0, 4]), torch.rand(4, 2))
    with pytest.raises(ValueError, match="rings_from_padded"):
        mo.rings_from_padded(torch.zeros(3, 5, 2), torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="counts outside"):
        mo.rings_from_padded(torch.zeros(2, 5, 2), torch.tensor([1, 6]))
    offs, xy = mo.rings_from_padded(torch.arange(20.0).view(2, 5, 2), torch.tensor([2, 5]))
    assert offs.tolist() == [0, 2, 7] and xy.shape == (7, 2) and xy[2].tolist() == [10.0, 11.0]
