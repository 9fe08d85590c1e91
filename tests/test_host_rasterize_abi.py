"""C-ABI surface of the ring rasterisation (CPU): the symbols exist with the documented signatures, the workspace size is
what the header says, the ABI version is still 32, bad arguments are rejected on the host with SEGGER_EINVAL and a message,
and no polygons returns 0 without a device -- nothing is launched by any call below (every pointer is a fake aligned
address that is never dereferenced).  The Python side raises every ValueError of its contract without a device, and
refuses CPU tensors naming the oracle file."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
PTRS = ("ring_offsets", "xy", "image", "n_covered", "n_won", "counters", "workspace")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def call(lib, P=10, V=50, H=16, W=24, sx=1.0, sy=1.0, tx=0.0, ty=0.0, predicate=1, overlap=0, block=8, reg_max=64, ws_bytes=1 << 20, **p):
    a = {name: FAKE for name in PTRS}
    a["labels"] = None
    a.update(p)
    return lib.segger_rasterize_rings(a["ring_offsets"], a["xy"], P, V, a["labels"], H, W, sx, sy, tx, ty, predicate, overlap, block,
                                      reg_max, a["image"], a["n_covered"], a["n_won"], a["counters"], a["workspace"], ws_bytes, None)


def test_symbols_signatures_constants_and_abi_version(lib):
    want = {"segger_rasterize_workspace_bytes": (C.c_int64, [i64]),
            "segger_rasterize_rings": (C.c_int, [vp, vp, i64, i64, vp, i32, i32, f64, f64, f64, f64, i32, i32, i32, i32, vp, vp, vp, vp,
                                                 vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION                  # purely additive
    import segger_amd
    from segger_amd import rasterize as rm
    assert segger_amd.rasterize is rm and segger_amd.rasterize_rings is rm.rasterize_rings
    assert rm.COUNTER_NAMES == ("n_pixels_set", "n_overlaps", "n_empty", "n_clipped", "n_degenerate", "n_large_tier", "n_blocks_filled")
    assert len(rm.COUNTER_NAMES) == _lib.RASTER_COUNTERS
    assert (_lib.RASTER_CONTAINS, _lib.RASTER_INTERSECTS) == (_lib.PJOIN_CONTAINS, _lib.PJOIN_INTERSECTS)
    assert rm.DEFAULT_BLOCK in (4, 8, 16)


def test_header_and_exports_declare_the_unit():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "segger_amd.h")).read()
    assert re.search(r"int segger_rasterize_rings\(const int64_t\* ring_offsets, const double\* xy,", header)
    assert "int64_t segger_rasterize_workspace_bytes(int64_t n_polygons);" in header
    for name, value in (("CONTAINS", 0), ("INTERSECTS", 1), ("LOWEST", 0), ("HIGHEST", 1), ("MAX_BLOCK", _lib.RASTER_MAX_BLOCK),
                        ("COUNTERS", _lib.RASTER_COUNTERS), ("ERR_OFFSETS", _lib.MORPH_ERR_OFFSETS), ("ERR_CAP", _lib.MORPH_ERR_CAP)):
        assert re.search(rf"#define SEGGER_RASTER_{name} {value}\b", header), name
    assert re.search(r"#define SEGGER_ABI_VERSION 32\b", header)
    assert "global: segger_*;" in open(os.path.join(root, "segger_amd", "csrc", "exports.map")).read()
    assert " rasterize.hip" in open(os.path.join(root, "segger_amd", "csrc", "Makefile")).read()


def test_workspace_size_is_what_the_header_says(lib):
    ws = lib.segger_rasterize_workspace_bytes

    def up(x):
        return (x + 255) // 256 * 256
    for P in (0, 1, 64, 65, 10 ** 6, (1 << 31) - 2):
        assert ws(P) == 256 + 2 * up(4 * P), P
    for bad in (-1, (1 << 31) - 1):
        assert ws(bad) == EINVAL and (b"negative" in lib.segger_last_error() or b"2^31" in lib.segger_last_error()), bad


def test_rejections(lib):
    err = lib.segger_last_error
    assert call(lib, P=-1) == EINVAL and b"negative" in err() and b"segger_rasterize_rings" in err()
    assert call(lib, P=(1 << 31) - 1) == EINVAL and b"2^31" in err()
    assert call(lib, V=-1) == EINVAL and b"negative n_vertices" in err()
    assert call(lib, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
    for shape in (dict(H=0), dict(W=0), dict(H=-4), dict(H=65536, W=32768), dict(H=46341, W=46341)):
        assert call(lib, **shape) == EINVAL and b"bad shape" in err(), shape
    for frame in (dict(sx=0.0), dict(sy=-0.0), dict(sx=math.inf), dict(sy=math.nan), dict(tx=math.nan), dict(ty=-math.inf)):
        assert call(lib, **frame) == EINVAL and b"bad frame" in err(), frame
    assert call(lib, predicate=2) == EINVAL and b"predicate 2" in err()
    assert call(lib, overlap=-1) == EINVAL and b"overlap -1" in err()
    for block in (0, -8, 3, 12, 64):
        assert call(lib, block=block) == EINVAL and b"power of two" in err(), block
    for reg_max in (1, 32, 65, -1):
        assert call(lib, reg_max=reg_max) == EINVAL and b"reg_max" in err(), reg_max
    for name in PTRS:
        assert call(lib, **{name: None}) == EINVAL and b"NULL" in err(), name
        assert call(lib, **{name: FAKE + 2}) == EINVAL and b"aligned" in err(), name
    for name in ("ring_offsets", "n_covered", "n_won", "counters"):
        assert call(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    assert call(lib, xy=FAKE + 8) == EINVAL and b"16-byte aligned" in err()
    assert call(lib, labels=FAKE + 2) == EINVAL and b"image and labels" in err()
    need = lib.segger_rasterize_workspace_bytes(10)
    assert call(lib, ws_bytes=need - 1) == EINVAL and b"workspace" in err() and str(need).encode() in err()
    assert call(lib, ws_bytes=0) == EINVAL and b"workspace" in err()


def test_no_polygons_returns_ok_without_a_device(lib):
    nothing = {name: None for name in PTRS}
    assert call(lib, P=0, V=0, ws_bytes=0, **nothing) == 0
    assert call(lib, P=0, V=0) == 0
    assert call(lib, P=0, sx=0.0) == EINVAL                          # the options are checked first


def test_python_side_raises_every_value_error_without_a_device():
    from segger_amd import rasterize_rings
    offs, xy = torch.tensor([0, 4]), torch.rand(4, 2, dtype=torch.float64)
    ok = dict(shape=(8, 8))

    def bad(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            rasterize_rings(*args, **{**ok, **kw})
    for shape in ((8,), (8, 8, 8), (0, 8), (8, -1), (8.0, 8), (True, 8), (65536, 32768), 8, None):
        bad("shape is", offs, xy, shape=shape)
    for scale in ((1.0,), (1.0, math.nan), (math.inf, 1.0), "ab", None, (1.0, 2.0, 3.0)):
        bad("scale is two finite numbers", offs, xy, scale=scale)
    for scale in ((0.0, 1.0), (1.0, -0.0)):
        bad("scale must be non-zero", offs, xy, scale=scale)
    for translation in ((0.0,), (math.nan, 0.0), (0.0, math.inf), None):
        bad("translation is two finite numbers", offs, xy, translation=translation)
    bad("predicate", offs, xy, predicate="within")
    bad("overlap", offs, xy, overlap="first")
    bad("_route", offs, xy, _route="small")
    for block in (0, 3, 64, 8.0, True, "8"):
        bad("_block", offs, xy, _block=block)
    for labels in (torch.ones(1, dtype=torch.int64), torch.ones(2, dtype=torch.int32), torch.ones(1, 1, dtype=torch.int32), [1]):
        bad("labels is an int32", offs, xy, labels=labels)
    bad("ring_offsets is an int64", torch.tensor([0.0, 4.0]), xy)
    bad("ring_offsets and xy are tensors", [0, 4], xy)
    bad("xy is a floating-point", offs, torch.zeros(4, 2, dtype=torch.int64))
    bad("xy is a floating-point", offs, torch.zeros(4, 3))
    many = _lib.MORPH_MAX_VERTS + 2
    bad("more than SEGGER_MORPH_MAX_VERTS", torch.tensor([0, many]), torch.rand(many, 2, dtype=torch.float64))


def test_python_side_refuses_cpu_tensors_and_names_the_oracle():
    from segger_amd import rasterize_rings
    offs, xy = torch.tensor([0, 4]), torch.rand(4, 2, dtype=torch.float64)
    for kw in ({}, dict(labels=torch.ones(1, dtype=torch.int32))):
        with pytest.raises(_lib.SeggerAmdError, match=r"MI355X only.*tests/rasterize_cases.py"):
            rasterize_rings(offs, xy, (8, 8), **kw)
    with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
        rasterize_rings(torch.tensor([0]), xy[:0], (8, 8))           # no polygons: still no CPU path
