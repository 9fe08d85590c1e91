"""Ring simplification and validity without a GPU: the oracles of tests/simplify_cases.py against rings worked by hand and
against properties that do not come from the oracle (subsequence, every dropped vertex within the tolerance of its chord,
simple in -> simple out by the exact oracle, equality with a separately written textbook Douglas-Peucker); the guard really
exercised (refusals >= 1 % of the sections visited over the random cases); the C-ABI surface of the four new symbols
(signatures, ABI version 32, the documented terms of the workspace size, every rejection of check_ring_call on fake pointers
that are never dereferenced); and the refusals of the Python wrappers, raised before the device is asked for."""
import ctypes as C

import numpy as np
import pytest
import torch

import simplify_cases as sc
from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


# ---------------------------------------------------------------- the oracles ---
def all_cases():
    out = [(name, np.array(ring, np.float64).reshape(-1, 2), tol) for name, (ring, tol) in sc.HAND.items()]
    out += [c for c in sc.boundary_rings() if len(c[1]) <= 300]     # the long ones are walked once, below
    for t in sc.TOLERANCES:
        out += [(f"random_{k}_{t}", r, t) for k, r in enumerate(sc.random_rings()[:16])]
    vor = sc.voronoi_rings()
    for t in sc.TOLERANCES + (sc.contour_tolerance(vor),):
        out += [(f"voronoi_{k}_{t}", r, t) for k, r in enumerate(vor[:12])]
    return out


def chord_of(kept, n, k):
    """the section ends between which the dropped vertex k lies"""
    ends = kept + [n]
    pos = int(np.searchsorted(ends, k))
    return ends[pos - 1], ends[pos]


def test_hand_cases_come_out_as_worked():
    for name, want in sc.HAND_KEPT.items():
        ring, tol = sc.HAND[name]
        assert sc.simplify_ring(ring, tol)[0] == want, name
    assert sc.simplify_ring(*sc.HAND["flat_abcb"])[1]["refused"] == 2          # both chords lie over the ring itself
    kept, st = sc.simplify_ring(sc.HAND["flat_abcb"][0], 1.0, preserve_topology=False)
    assert kept == [0, 1, 2, 3] and st["kind"] == "restored"
    assert sc.simplify_ring(*sc.HAND["all_equal"])[1]["kind"] == "restored"
    for name in ("n0", "n1", "n2", "n2_closed"):
        assert sc.simplify_ring(*sc.HAND[name])[1]["kind"] == "passed", name


@pytest.mark.parametrize("name", ["u_crossed", "u_tip_on_chord"])
def test_guard_refuses_where_the_classical_algorithm_self_intersects(name):
    ring, tol = sc.HAND[name]
    pts = np.array(ring, np.float64)
    assert sc.ring_simple_exact(pts, fractions=True)[0]
    classical = sc.textbook_dp(ring, tol)
    assert not sc.ring_simple_exact(pts[classical], fractions=True)[0]          # the chord y = 0 meets the peninsula
    kept, st = sc.simplify_ring(ring, tol)
    assert st["refused"] >= 1 and sc.ring_simple_exact(pts[kept], fractions=True)[0]
    assert len(kept) < len(ring)                                                # and it still simplified something


def test_oracle_properties_on_every_case():
    for name, ring, tol in all_cases():
        pts = sc.open_ring(ring)
        n = len(pts)
        for preserve in (True, False):
            kept, st = sc.simplify_ring(ring, tol, preserve)
            assert kept == sorted(set(kept)) and all(0 <= k < n for k in kept), name
            assert (kept[:1] == [0]) if n else kept == [], name
            if st["kind"]:
                assert kept == list(range(n)), name
                continue
            v = np.vstack([pts - pts[0], np.zeros((1, 2))])
            for k in sorted(set(range(n)) - set(kept)):
                i, j = chord_of(kept, n, k)
                assert sc._dist2(v[k], v[i], v[j]) <= tol * tol, (name, k)
                if tol == 0.0:                                       # only vertices ON their chord go
                    assert sc._dist2(v[k], v[i], v[j]) == 0.0, (name, k)
            if not preserve:
                assert kept == sc.textbook_dp(ring, tol), name
        try:
            simple_in = sc.ring_simple_exact(pts)[0]
        except AssertionError:                                       # not on the grid (the comb): nothing exact to say
            continue
        if simple_in:
            kept = sc.simplify_ring(ring, tol)[0]
            assert sc.ring_simple_exact(pts[kept])[0], name


def test_guard_is_exercised_by_the_random_cases():
    sections = refused = 0
    for t in sc.TOLERANCES:
        for r in sc.random_rings():
            st = sc.simplify_ring(r, t)[1]
            sections += st["sections"]
            refused += st["refused"]
    assert refused >= 0.01 * sections, (refused, sections)


def test_long_rings_and_the_comb():
    for name, ring, tol in sc.boundary_rings():
        if len(ring) < 4095:
            continue
        kept, st = sc.simplify_ring(ring, tol)
        assert kept[0] == 0 and 3 <= len(kept) <= len(ring), name
        if name.startswith("comb"):
            # the stack of pending right halves nearly n deep: all but the first hundred or so vertices, whose radius is
            # still comparable with the translation to vertex 0 and which split less regularly
            assert st["max_pending"] >= len(ring) - 128, (name, st)
            assert kept == list(range(len(ring)))
    assert sc.simplify_ring(sc.comb_ring(257), 0.0)[1]["max_pending"] >= 257 - 128


def test_exact_touch_agrees_with_the_orientation_form():
    rng = np.random.default_rng(3)
    segs = rng.integers(-3, 4, (4000, 4, 2))                         # a tiny grid: overlaps, shared ends, points abound
    segs[:400, 1] = segs[:400, 0]                                    # zero-length segments
    segs[200:600, 3] = segs[200:600, 2]
    seen = set()
    for a, b, c, d in segs:
        want = sc.touch_exact(a, b, c, d)
        assert bool(sc.touch_many(a, b, c[None], d[None])[0]) == want, (a, b, c, d)
        assert bool(sc.touch_many(a.astype(np.float64), b.astype(np.float64), c[None].astype(np.float64),
                                  d[None].astype(np.float64))[0]) == want
        assert sc.touch_exact(c, d, a, b) == want
        sh = sc.shared_exact(a, b, c, d)
        seen.add((None if sh is None else sh[0], want))
    assert seen == {(None, False), ("point", False), ("point", True), ("overlap", True)}
    P = lambda *p: np.array(p)
    assert not sc.touch_exact(P(0, 0), P(2, 0), P(2, 0), P(2, 5))    # a shared endpoint
    assert sc.touch_exact(P(0, 0), P(2, 0), P(1, 0), P(1, 5))        # an endpoint in the other's interior
    assert sc.touch_exact(P(0, 0), P(2, 0), P(2, 0), P(1, 0))        # a fold-back
    assert sc.touch_exact(P(0, 0), P(2, 0), P(2, 0), P(0, 0))        # the same segment
    assert not sc.touch_exact(P(1, 1), P(1, 1), P(1, 1), P(1, 1))    # two points
    assert sc.touch_exact(P(1, 0), P(1, 0), P(0, 0), P(2, 0))        # a point in a segment's interior


def test_simplicity_oracle():
    want = {"square_midpoints": (sc.OK, -1, -1), "flat_abcb": (sc.TOUCH, 0, 3), "all_equal": (sc.TOO_FEW, -1, -1),
            "neck_revisits_vertex": (sc.OK, -1, -1), "n2": (sc.TOO_FEW, -1, -1), "n3": (sc.OK, -1, -1),
            "consecutive_duplicates": (sc.OK, -1, -1), "u_crossed": (sc.OK, -1, -1), "n0": (sc.TOO_FEW, -1, -1)}
    for name, reason in want.items():
        for fractions in (False, True):
            assert sc.ring_simple_exact(sc.HAND[name][0], fractions) == (reason[0] == sc.OK, reason), name
    assert sc.ring_simple_exact([(0, 0), (5, 0), (5, 0), (0, 0), (0, 0)])[1] == (sc.TOO_FEW, -1, -1)   # two distinct vertices
    assert sc.ring_simple_exact([(0, 0), (4, 0), (4, 4), (2, -1)])[1] == (sc.TOUCH, 0, 2)              # a proper crossing
    for seed in range(8):                                            # coarse ragged stars: some simple, some not
        r = sc.star_ring(24, 50 + seed, r_lo=0.1, scale=9.0)
        assert sc.ring_simple_exact(r) == sc.ring_simple_exact(r, fractions=True), seed


# ---------------------------------------------------------------- the C ABI ---
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def mark(lib, P=3, V=20, stride=0, preserve=1, small=256, ws_bytes=1 << 20, **p):
    a = dict(ring_offsets=FAKE, xy=FAKE, tolerance=FAKE, out_offsets=FAKE, counters=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_simplify_rings_mark(a["ring_offsets"], a["xy"], P, V, a["tolerance"], stride, preserve, small, a["out_offsets"],
                                          a["counters"], a["workspace"], ws_bytes, None)


def emit(lib, P=3, V=20, capacity=10, ws_bytes=1 << 20, **p):
    a = dict(ring_offsets=FAKE, xy=FAKE, out_offsets=FAKE, xy_out=FAKE, vertex_index=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_simplify_rings_emit(a["ring_offsets"], a["xy"], P, V, a["out_offsets"], a["xy_out"], a["vertex_index"], capacity,
                                          a["workspace"], ws_bytes, None)


def simple(lib, P=3, V=20, small=256, ws_bytes=1 << 20, **p):
    a = dict(ring_offsets=FAKE, xy=FAKE, ok=FAKE, reason=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_rings_simple(a["ring_offsets"], a["xy"], P, V, a["ok"], a["reason"], small, a["workspace"], ws_bytes, None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_simplify_rings_workspace_bytes": (C.c_int64, [i64, i64]),
            "segger_simplify_rings_mark": (C.c_int, [vp, vp, i64, i64, vp, i64, i32, i32, vp, vp, vp, i64, vp]),
            "segger_simplify_rings_emit": (C.c_int, [vp, vp, i64, i64, vp, vp, vp, i64, vp, i64, vp]),
            "segger_rings_simple": (C.c_int, [vp, vp, i64, i64, vp, vp, i32, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION                  # purely additive
    assert (_lib.SIMPLIFY_SMALL_VERTS, _lib.SIMPLIFY_COUNTERS, _lib.SIMPLIFY_ERR_TOL) == (256, 8, 4)
    assert (_lib.RING_OK, _lib.RING_TOO_FEW, _lib.RING_TOUCH) == (sc.OK, sc.TOO_FEW, sc.TOUCH)
    import segger_amd
    from segger_amd import simplify
    assert segger_amd.simplify_rings is simplify.simplify_rings and segger_amd.rings_simple is simplify.rings_simple
    assert segger_amd.contour_tolerance is simplify.contour_tolerance
    assert simplify.COUNTER_NAMES == sc.COUNTERS and len(simplify.COUNTER_NAMES) == _lib.SIMPLIFY_COUNTERS - 1


def test_workspace_size_has_the_documented_terms(lib):
    def up(x):
        return (x + 255) // 256 * 256
    size = lib.segger_simplify_rings_workspace_bytes
    for P, V in ((0, 0), (1, 3), (3, 20), (1000, 99999), (1 << 20, 100 << 20), (5, 0)):
        assert size(P, V) == 256 + 2 * up(4 * P) + up(16 * P) + up(V), (P, V)
    for P, V in ((-1, 0), (0, -1), ((1 << 31) - 1, 0)):
        assert size(P, V) == EINVAL, (P, V)
    assert b"2^31" in lib.segger_last_error()


def test_rejections(lib):
    err = lib.segger_last_error
    for fn, own8, own16 in ((mark, ("tolerance", "out_offsets", "counters"), ()), (emit, ("out_offsets", "vertex_index"), ("xy_out",)),
                            (simple, (), ())):
        assert fn(lib, P=-1) == EINVAL and b"negative" in err()
        assert fn(lib, V=-1) == EINVAL and b"negative" in err()
        assert fn(lib, P=(1 << 31) - 1) == EINVAL and b"2^31" in err()
        assert fn(lib, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
        for name in ("ring_offsets", "workspace") + own8 + own16:
            assert fn(lib, **{name: None}) == EINVAL and b"NULL pointer" in err(), (fn.__name__, name)
        assert fn(lib, xy=None) == EINVAL and b"NULL xy" in err()
        for name in ("ring_offsets",) + own8:
            assert fn(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), (fn.__name__, name)
        for name in ("xy",) + own16:
            assert fn(lib, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), (fn.__name__, name)
        assert fn(lib, workspace=FAKE + 64) == EINVAL and b"256-byte aligned" in err()
        need = lib.segger_simplify_rings_workspace_bytes(3, 0 if fn is simple else 20)
        assert fn(lib, ws_bytes=need - 1) == EINVAL and str(need).encode() in err()
    for s in (-1, 2):
        assert mark(lib, stride=s) == EINVAL and b"tolerance_stride" in err()
    for fn in (mark, simple):
        for s in (-1, 257):
            assert fn(lib, small=s) == EINVAL and b"small_max_verts" in err()
    for name in ("ok", "reason"):
        assert simple(lib, **{name: None}) == EINVAL and b"NULL pointer" in err()
    assert simple(lib, reason=FAKE + 2) == EINVAL and b"4-byte aligned" in err()
    assert emit(lib, capacity=-1) == EINVAL and b"negative capacity" in err()


def test_empty_input_returns_ok_without_a_device(lib):
    none = dict(ring_offsets=None, xy=None, workspace=None)
    assert mark(lib, P=0, V=0, ws_bytes=0, tolerance=None, out_offsets=None, counters=None, **none) == 0
    assert emit(lib, P=0, V=0, ws_bytes=0, out_offsets=None, xy_out=None, vertex_index=None, **none) == 0
    assert emit(lib, capacity=0, ws_bytes=0, out_offsets=None, xy_out=None, vertex_index=None, **none) == 0
    assert simple(lib, P=0, V=0, ws_bytes=0, ok=None, reason=None, **none) == 0


# ---------------------------------------------------------------- the wrappers ---
def test_python_side_refusals():
    from segger_amd import contour_tolerance, rings_simple, simplify_rings
    off, xy = (torch.from_numpy(t) for t in sc.csr([sc.HAND["n3"][0], sc.HAND["square_midpoints"][0]]))
    for bad in (-1.0, float("inf"), float("nan"), torch.tensor(-0.5), torch.tensor(float("nan"))):
        with pytest.raises(ValueError, match="finite and >= 0"):
            simplify_rings(off, xy, bad)
    for bad in ("1", None, True, torch.tensor(1), torch.zeros(2, 2)):
        with pytest.raises(ValueError, match="tolerance is a float"):
            simplify_rings(off, xy, bad)
    with pytest.raises(ValueError, match="3 entries for 2 polygons"):
        simplify_rings(off, xy, torch.zeros(3, dtype=torch.float64))
    for bad in ("small", 0, "LARGE"):
        with pytest.raises(ValueError, match="_route"):
            simplify_rings(off, xy, 1.0, _route=bad)
        with pytest.raises(ValueError, match="_route"):
            rings_simple(off, xy, _route=bad)
    for fn in (lambda o, x: simplify_rings(o, x, 1.0), rings_simple, contour_tolerance):
        with pytest.raises(ValueError, match="ring_offsets"):
            fn(off.float(), xy)
        with pytest.raises(ValueError, match="xy"):
            fn(off, xy[:, :1])
        with pytest.raises(ValueError, match="tensors"):
            fn(off.numpy(), xy)
    for bad in (-1.0, float("nan"), "x", True):
        with pytest.raises(ValueError, match="frac"):
            contour_tolerance(off, xy, bad)
    long_off, long_xy = (torch.from_numpy(t) for t in sc.csr([sc.HAND["n3"][0], sc.star_ring(sc.MAX_VERTS + 1, 5)]))
    for fn in (lambda o, x: simplify_rings(o, x, 1.0), rings_simple):
        with pytest.raises(ValueError, match="polygon 1 has 4097 vertices"):   # n = 4097 is refused, and named
            fn(long_off, long_xy)
    for fn in (lambda: simplify_rings(off, xy, 1.0), lambda: rings_simple(off, xy), lambda: contour_tolerance(off, xy),
               lambda: simplify_rings(off, xy, torch.tensor([1.0, 2.0], dtype=torch.float64), preserve_topology=False)):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):           # as the rest of the product: no CPU fallback
            fn()
