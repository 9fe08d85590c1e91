"""The C-ABI surface of segger_fragments_update / segger_fragments_finalize without a GPU: the symbols and their signatures,
ABI version 32 (purely additive), and every rejection on fake pointers that are never dereferenced -- answered with an
error code and a message, nothing launched."""
import ctypes as C

import pytest

from segger_amd import _lib

EINVAL, EWORKSPACE_OR_EINVAL = -1, (-1, -4)
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def update(lib, **p):
    a = dict(z=FAKE, ld_z=8, channels=8, dtype=0, similarity=None, edge_keep=None, src=FAKE, dst=FAKE, n_edges=10, tx_index=FAKE,
             mask=FAKE, n_nodes=5, unassigned=FAKE, n_transcripts=100, min_similarity=0.5, parent=FAKE, counters=FAKE)
    a.update(p)
    return lib.segger_fragments_update(*[a[k] for k in ("z", "ld_z", "channels", "dtype", "similarity", "edge_keep", "src", "dst",
                                                        "n_edges", "tx_index", "mask", "n_nodes", "unassigned", "n_transcripts",
                                                        "min_similarity", "parent", "counters")], None)


def workspace_bytes(n):
    up = lambda x: (x + 255) // 256 * 256                             # noqa: E731
    return up(4 * n) + up(8 * ((n + 2047) // 2048 + 1))


def finalize(lib, **p):
    a = dict(parent=FAKE, unassigned=FAKE, n=100, min_size=5, first_id=0, fragment=FAKE, root=FAKE, size=FAKE, capacity=20,
             counters=FAKE, workspace=FAKE, ws_bytes=1 << 20)
    a.update(p)
    return lib.segger_fragments_finalize(*[a[k] for k in ("parent", "unassigned", "n", "min_size", "first_id", "fragment", "root", "size",
                                                          "capacity", "counters", "workspace", "ws_bytes")], None)


def test_symbols_signatures_and_abi_version(lib):
    sigs = {"segger_fragments_update": (C.c_int, [vp, i64, i32, i32, vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, f32, vp, vp, vp]),
            "segger_fragments_finalize": (C.c_int, [vp, vp, i64, i64, i64, vp, vp, vp, i64, vp, vp, i64, vp])}
    for name, sig in sigs.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION           # purely additive
    assert (_lib.FRAGMENTS_COUNTERS, _lib.FRAGMENTS_CHUNK, _lib.FRAGMENTS_MAX_CHANNELS) == (8, 2048, 1024)
    import segger_amd
    from segger_amd import fragments
    for name in ("FragmentAccumulator", "fragment_cells", "connected_components", "unassigned_mask", "merge_fragments"):
        assert getattr(segger_amd, name) is getattr(fragments, name), name
    assert len(fragments.COUNTER_NAMES) == _lib.FRAGMENTS_COUNTERS and fragments.MAX_CHANNELS == 1024
    assert fragments._workspace_bytes(100) == workspace_bytes(100) and fragments._workspace_bytes(1 << 20) == workspace_bytes(1 << 20)


def test_update_rejections(lib):
    err = lib.segger_last_error
    assert update(lib, n_edges=-1) == EINVAL and b"negative" in err()
    assert update(lib, n_nodes=-1) == EINVAL and b"negative" in err()
    for n in (0, -3, 1 << 31):
        assert update(lib, n_transcripts=n) == EINVAL and b"n_transcripts outside [1, 2^31)" in err()
    assert update(lib, n_nodes=1 << 31) == EINVAL and b"2^31 nodes" in err()
    assert update(lib, similarity=FAKE) == EINVAL and b"both z and similarity" in err()
    assert update(lib, min_similarity=float("nan")) == EINVAL and b"NaN" in err()
    for c in (0, -1, 1025):
        assert update(lib, channels=c, ld_z=2048) == EINVAL and b"channels" in err()
    for d in (-1, 3):
        assert update(lib, dtype=d) == EINVAL and b"dtype" in err()
    assert update(lib, ld_z=7) == EINVAL and b"ld_z < channels" in err()
    assert update(lib, z=FAKE + 2) == EINVAL and b"element size" in err()
    assert update(lib, z=FAKE + 1, dtype=1) == EINVAL and b"element size" in err()
    for name in ("src", "dst", "unassigned", "parent", "counters"):
        assert update(lib, **{name: None}) == EINVAL and b"NULL pointer" in err(), name
    assert update(lib, n_nodes=0) == EINVAL and b"n_nodes = 0" in err()
    for name in ("src", "dst", "tx_index", "counters"):
        assert update(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    assert update(lib, parent=FAKE + 2) == EINVAL and b"4-byte aligned" in err()
    assert update(lib, z=None, similarity=FAKE + 2) == EINVAL and b"4-byte aligned" in err()


def test_update_without_edges_returns_ok_without_a_device(lib):
    assert update(lib, n_edges=0, src=None, dst=None, tx_index=None, mask=None, unassigned=None, parent=None, counters=None) == 0
    assert update(lib, n_edges=0, z=None, channels=0, ld_z=0) == 0


def test_finalize_rejections(lib):
    err = lib.segger_last_error
    for n in (0, -1, 1 << 31):
        assert finalize(lib, n=n) == EINVAL and b"n_transcripts outside [1, 2^31)" in err()
    for m in (0, -5):
        assert finalize(lib, min_size=m) == EINVAL and b"min_size" in err()
    for f in (-1, (1 << 63) - 50):
        assert finalize(lib, first_id=f) == EINVAL and b"first_id" in err()
    assert finalize(lib, capacity=-1) == EINVAL and b"negative capacity" in err()
    assert finalize(lib, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
    for name in ("parent", "unassigned", "fragment", "counters", "workspace"):
        assert finalize(lib, **{name: None}) == EINVAL and b"NULL pointer" in err(), name
    for name in ("root", "size"):
        assert finalize(lib, **{name: None}) == EINVAL and b"NULL root or size" in err(), name
    for name in ("fragment", "counters"):
        assert finalize(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name
    for name in ("parent", "root", "size"):
        assert finalize(lib, **{name: FAKE + 2}) == EINVAL and b"4-byte aligned" in err(), name
    assert finalize(lib, workspace=FAKE + 64) == EINVAL and b"256-byte aligned" in err()
    for n in (1, 100, 2048, 2049, 1 << 20):
        need = workspace_bytes(n)
        assert finalize(lib, n=n, ws_bytes=need - 1) in EWORKSPACE_OR_EINVAL and str(need).encode() in err(), n
