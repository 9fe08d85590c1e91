"""C-ABI surface of the quadtree entry points (CPU): bad arguments are rejected on the host with a negative code and a
message -- nothing is launched -- and the workspace size grows with the number of points."""
import ctypes

import pytest

from segger_amd import _lib

EINVAL, EWORKSPACE = -1, -4
FAKE = 0x1000                     # a non-NULL, 8-byte aligned address: never dereferenced, every call below is rejected


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def build(lib, n=1000, depth=10, max_size=32, cap=100, cell=1.0, points=FAKE, out=FAKE, ws=FAKE, ws_bytes=1 << 40):
    return lib.segger_quadtree_build(points, n, 0.0, 0.0, cell, depth, max_size, cap, out, out, out, out, out, out, out,
                                     ws, ws_bytes, None)


def label(lib, n=1000, depth=10, n_leaf=10, cell=1.0, points=FAKE, tab=FAKE, out=FAKE, x1=100.0):
    return lib.segger_quadtree_label(points, n, 0.0, 0.0, x1, 100.0, cell, depth, tab, tab, tab, tab, n_leaf, out, None)


def test_workspace_bytes_rejects_bad_sizes_and_is_monotone(lib):
    ws = lib.segger_quadtree_workspace_bytes
    for args, word in (((1 << 31, 10, 32, 100), b"2^31"), ((0, 10, 32, 100), b"point"), ((1000, 16, 32, 100), b"depth"),
                       ((1000, 0, 32, 100), b"depth"), ((1000, 10, 0, 100), b"max_size"), ((1000, 10, 32, 0), b"capacity")):
        assert ws(*args) == EINVAL and word in lib.segger_last_error(), args
    sizes = [ws(n, 15, 50, min(n, 4 + 42 * (n // 51))) for n in (1, 2, 255, 256, 257, 10_000, 1_000_000, 50_000_000)]
    assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])), sizes   # monotone (segments are rounded up to 256 bytes)
    assert sizes[2] > sizes[0] and sizes[5] > sizes[4] and sizes[7] > sizes[6] > sizes[5]
    assert sizes[-1] >= 2 * 4 * 50_000_000                            # two key arrays at the very least


def test_build_rejects_bad_arguments(lib):
    assert build(lib, n=1 << 31) == EINVAL and b"2^31" in lib.segger_last_error()
    assert build(lib, n=0) == EINVAL and b"point" in lib.segger_last_error()
    assert build(lib, depth=16) == EINVAL and b"depth" in lib.segger_last_error()
    assert build(lib, max_size=0) == EINVAL and b"max_size" in lib.segger_last_error()
    assert build(lib, cap=0) == EINVAL and b"capacity" in lib.segger_last_error()
    assert build(lib, points=None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert build(lib, out=None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert build(lib, points=FAKE + 4) == EINVAL and b"aligned" in lib.segger_last_error()
    assert build(lib, cell=3.0) == EINVAL and b"power of two" in lib.segger_last_error()
    assert build(lib, cell=0.5) == EINVAL and b"power of two" in lib.segger_last_error()
    assert build(lib, ws=None) == EWORKSPACE and b"workspace" in lib.segger_last_error()
    assert build(lib, ws_bytes=16) == EWORKSPACE and b"workspace" in lib.segger_last_error()


def test_label_rejects_bad_arguments(lib):
    assert label(lib, n=1 << 31) == EINVAL and b"2^31" in lib.segger_last_error()
    assert label(lib, n=-1) == EINVAL and b"negative" in lib.segger_last_error()
    assert label(lib, depth=16) == EINVAL and b"depth" in lib.segger_last_error()
    assert label(lib, n_leaf=0) == EINVAL and b"leaf count" in lib.segger_last_error()
    assert label(lib, points=None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert label(lib, tab=None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert label(lib, out=None) == EINVAL and b"NULL" in lib.segger_last_error()
    assert label(lib, cell=6.0) == EINVAL and b"power of two" in lib.segger_last_error()
    assert label(lib, x1=-1.0) == EINVAL and b"root box" in lib.segger_last_error()
    assert label(lib, n=0, points=None, out=None) == 0                # nothing to label: nothing is launched
