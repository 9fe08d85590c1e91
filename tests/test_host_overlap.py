"""The polygon overlap join without a GPU: the contract's area formula in exact rationals EQUAL to an independent exact
oracle (Sutherland-Hodgman clipping by a convex polygon), the identities the formula must satisfy, exact in Fraction, the
exact predicate on the hand cases, the C-ABI surface of the three new symbols (signatures, ABI version 32, constants, the
documented and monotone workspace size, rejections on fake pointers that are never dereferenced) and the refusals of the
Python wrappers, raised before the device is asked for."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import overlap_cases as oc
from segger_amd import _lib

EINVAL = -1
FAKE = 0x1000                     # a non-NULL, 256-byte aligned address
vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double


# ---------------------------------------------------------------- the oracles ---
def test_formula_equals_exact_clipping_on_random_pairs():
    pairs = oc.random_pairs(210)
    assert len(pairs) >= 200
    positive = 0
    for a, b in pairs:
        for aa in (a, a[::-1]):
            for bb in (b, b[::-1]):
                v, T, S = oc.area_formula(aa, bb)
                assert v == oc.clip_area(aa, bb)
                assert 0 <= v <= S and (T > 0) == (S > 0)
        positive += v > 0
    assert positive >= 100                                           # the pairs do overlap


def test_hand_cases():
    for name, (a, b, area, hit) in oc.HAND.items():
        assert oc.intersects_exact(a, b) == hit == oc.intersects_exact(b, a), name
        if area is not None:
            assert oc.area_formula(a, b)[0] == area == oc.area_formula(b, a)[0], name
            assert abs(oc.area_formula_f64(a, b)[0] - area) < 1e-12, name


def test_identities_are_exact():
    rings = [oc.star(n, 40 + n, scale=300) for n in (3, 5, 11, 24)] + [oc.convex(9, 3, scale=200, centre=(40, -30))]
    for a in rings:
        area = Fraction(abs(oc.shoelace2(oc.ints(a))), 2)
        assert oc.area_formula(a, a)[0] == area                      # A & A
        for b in rings:
            v = oc.area_formula(a, b)[0]
            assert v == oc.area_formula(b, a)[0]                     # symmetry
            for aa in (a[::-1], np.roll(a, 2, 0), np.roll(a[::-1], -1, 0)):     # orientation, start vertex
                assert oc.area_formula(aa, b)[0] == v == oc.area_formula(b, aa)[0]
        # two polygons that partition a rectangle containing A: a slanted cut
        lo, hi = a.min(0) - 5, a.max(0) + 7
        left = np.array([(lo[0], lo[1]), (lo[0] + 100, lo[1]), (hi[0] - 90, hi[1]), (lo[0], hi[1])])
        right = np.array([(lo[0] + 100, lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (hi[0] - 90, hi[1])])
        assert oc.area_formula(a, left)[0] + oc.area_formula(a, right)[0] == area
        inner = oc.rect(-20, -20, 25, 30) * 0.1 // 1                 # nested: a small rectangle round the star's centre
        if all(oc.inside(p, oc.ints(a)) for p in oc.ints(inner)) and not any(
                oc.segments_meet(p, q, r, s) for p, q in zip(oc.ints(a), oc.ints(np.roll(a, -1, 0)))
                for r, s in zip(oc.ints(inner), oc.ints(np.roll(inner, -1, 0)))):
            assert oc.area_formula(a, inner)[0] == Fraction(abs(oc.shoelace2(oc.ints(inner))), 2)
    assert oc.area_formula(oc.SQUARE * 7, oc.rect(2, 3, 6, 8))[0] == 20            # nested gives the inner area
    for name in ("shared_edge", "shared_vertex", "collinear_overlap"):
        a, b = oc.HAND[name][:2]
        assert oc.area_formula(a, b)[0] == 0 and oc.intersects_exact(a, b)
    for name in ("boxes_meet_disjoint", "l_and_notch"):
        a, b = oc.HAND[name][:2]
        assert len(oc.bbox_pairs([a], [b])) == 1 and oc.area_formula(a, b)[0] == 0 and not oc.intersects_exact(a, b)


def test_float64_formula_and_expected_join_agree_with_the_exact_one():
    a, b = oc.scene(40, 1, extent=600), oc.scene(40, 2, extent=600)
    want = oc.expected(a, b)
    assert 0 < want["pairs"].shape[1] < len(want["candidates"]) < 1600
    for (i, j), area, tol in zip(want["pairs"].T, want["area"], want["tol"]):
        assert abs(oc.area_formula_f64(a[i], b[j])[0] - area) <= tol
    m = oc.match_numpy(want["pairs"], want["area"], np.array([abs(oc.shoelace2(oc.ints(r))) / 2 for r in a]),
                       np.array([abs(oc.shoelace2(oc.ints(r))) / 2 for r in b]))
    assert (m["iou"] <= 1).all() and (m["best_b"][m["n_overlapping"] == 0] == -1).all()


# ---------------------------------------------------------------- the C ABI ---
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def cand(lib, Pa=3, Va=20, Pb=4, Vb=30, cell=1.0, nx=4, ny=4, ws_bytes=1 << 20, x0=0.0, **p):
    a = dict(ring_offsets_a=FAKE, xy_a=FAKE, ring_offsets_b=FAKE, xy_b=FAKE, n_candidates=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_polygon_overlap_candidates(a["ring_offsets_a"], a["xy_a"], Pa, Va, a["ring_offsets_b"], a["xy_b"], Pb, Vb, x0, 0.0,
                                                 cell, nx, ny, a["n_candidates"], a["workspace"], ws_bytes, None)


def pairs(lib, Pa=3, Va=20, Pb=4, Vb=30, cell=1.0, nx=4, ny=4, ws_bytes=1 << 20, x0=0.0, capacity=10, reg=64, small=256, **p):
    a = dict(ring_offsets_a=FAKE, xy_a=FAKE, ring_offsets_b=FAKE, xy_b=FAKE, area_a=FAKE, area_b=FAKE, n_candidates=FAKE, candidates=FAKE,
             intersects=FAKE, area=FAKE, workspace=FAKE)
    a.update(p)
    return lib.segger_polygon_overlap_pairs(a["ring_offsets_a"], a["xy_a"], Pa, Va, a["ring_offsets_b"], a["xy_b"], Pb, Vb, x0, 0.0, cell,
                                            nx, ny, a["area_a"], a["area_b"], a["n_candidates"], a["candidates"], a["intersects"], a["area"],
                                            capacity, reg, small, a["workspace"], ws_bytes, None)


def test_symbols_signatures_and_abi_version(lib):
    want = {"segger_polygon_overlap_workspace_bytes": (C.c_int64, [i64, i64, i32, i32]),
            "segger_polygon_overlap_candidates": (C.c_int, [vp, vp, i64, i64, vp, vp, i64, i64, f64, f64, f64, i32, i32, vp, vp, i64, vp]),
            "segger_polygon_overlap_pairs": (C.c_int, [vp, vp, i64, i64, vp, vp, i64, i64, f64, f64, f64, i32, i32, vp, vp, vp, vp, vp, vp,
                                                       i64, i32, i32, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.EXPORTS[name] == sig, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION                  # purely additive
    assert (_lib.OVERLAP_SMALL_VERTS, _lib.OVERLAP_WIDE_CELLS) == (oc.SMALL_VERTS, oc.WIDE_CELLS) == (256, 64)
    import segger_amd
    from segger_amd import overlap
    assert segger_amd.polygon_overlaps is overlap.polygon_overlaps and segger_amd.polygons_in_polygons is overlap.polygons_in_polygons
    assert segger_amd.match_polygons is overlap.match_polygons and overlap.COUNTER_NAMES == oc.COUNTERS


def test_workspace_size_has_the_documented_terms_and_is_monotone(lib):
    def up(x):
        return (x + 255) // 256 * 256
    size = lib.segger_polygon_overlap_workspace_bytes
    cases = ((0, 0, 1, 1), (1, 1, 1, 1), (3, 4, 4, 4), (1000, 999, 31, 33), (50000, 50000, 224, 224), (1 << 20, 5, 1000, 1000))
    for Pa, Pb, nx, ny in cases:
        c = nx * ny
        want = 256 + 2 * up(4 * Pa) + 2 * up(4 * Pb) + up(32 * Pa) + up(32 * Pb) + up(16 * Pa) + up(16 * Pb) + up(4 * Pa) + up(4 * Pb) + \
            up(4 * (c + 1)) + up(4 * c) + up(4 * 64 * Pb) + up(8 * (Pa + Pb + 1))
        assert size(Pa, Pb, nx, ny) == want, (Pa, Pb, nx, ny)
        for more in ((Pa + 100, Pb, nx, ny), (Pa, Pb + 100, nx, ny), (Pa, Pb, nx + 9, ny), (Pa, Pb, nx, ny + 9)):
            assert size(*more) >= want
    for bad in ((-1, 0, 1, 1), (0, -1, 1, 1), ((1 << 31) // 64, 0, 1, 1), (0, (1 << 31) // 64, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0),
                (1, 1, 1 << 16, 1 << 15)):
        assert size(*bad) == EINVAL, bad
    assert b"bad grid" in lib.segger_last_error()


def test_rejections(lib):
    err = lib.segger_last_error
    for fn, own in ((cand, ("n_candidates",)), (pairs, ("n_candidates", "candidates", "intersects", "area"))):
        assert fn(lib, Pa=-1) == EINVAL and b"negative" in err()
        assert fn(lib, Vb=-1) == EINVAL and b"negative" in err()
        assert fn(lib, Pb=1 << 26) == EINVAL and b"2^31" in err()
        assert fn(lib, nx=0) == EINVAL and b"bad grid" in err()
        assert fn(lib, cell=0.0) == EINVAL and b"bad grid" in err()
        assert fn(lib, x0=float("nan")) == EINVAL and b"bad grid" in err()
        assert fn(lib, ws_bytes=-1) == EINVAL and b"negative workspace_bytes" in err()
        for name in ("ring_offsets_a", "ring_offsets_b", "xy_b", "workspace") + own:
            assert fn(lib, **{name: None}) == EINVAL and b"NULL pointer" in err(), (fn.__name__, name)
        assert fn(lib, xy_a=None) == EINVAL and b"NULL xy" in err()
        for name in ("ring_offsets_a", "ring_offsets_b", "n_candidates"):
            assert fn(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), (fn.__name__, name)
        for name in ("xy_a", "xy_b"):
            assert fn(lib, **{name: FAKE + 8}) == EINVAL and b"16-byte aligned" in err(), (fn.__name__, name)
        assert fn(lib, workspace=FAKE + 64) == EINVAL and b"256-byte aligned" in err()
        need = lib.segger_polygon_overlap_workspace_bytes(3, 4, 4, 4)
        assert fn(lib, ws_bytes=need - 1) == EINVAL and str(need).encode() in err()
    assert pairs(lib, capacity=-1) == EINVAL and b"negative capacity" in err()
    for kw in (dict(reg=-1), dict(reg=65)):
        assert pairs(lib, **kw) == EINVAL and b"reg_max_verts" in err()
    for kw in (dict(small=-1), dict(small=257)):
        assert pairs(lib, **kw) == EINVAL and b"small_max_verts" in err()
    assert pairs(lib, area_a=None) == EINVAL and b"NULL pointer" in err()       # both areas, or neither
    for name in ("candidates", "area", "area_a"):
        assert pairs(lib, **{name: FAKE + 4}) == EINVAL and b"8-byte aligned" in err(), name


def test_empty_input_returns_ok_without_a_device(lib):
    none = dict(ring_offsets_a=None, xy_a=None, ring_offsets_b=None, xy_b=None, workspace=None, n_candidates=None)
    more = dict(candidates=None, intersects=None, area=None, area_a=None, area_b=None)
    for kw in (dict(Pa=0, Va=0), dict(Pb=0, Vb=0)):
        assert cand(lib, ws_bytes=0, **kw, **none) == 0
        assert pairs(lib, ws_bytes=0, **kw, **none, **more) == 0
    assert pairs(lib, capacity=0, **more) == 0                       # nothing to write: returns before anything is launched


# ---------------------------------------------------------------- the wrappers ---
def test_python_side_refusals():
    from segger_amd import match_polygons, polygon_overlaps, polygons_in_polygons
    off, xy = (torch.from_numpy(t) for t in oc.csr([oc.SQUARE, oc.star(5, 1)]))
    with pytest.raises(ValueError, match="'contains' is not built: deciding it exactly needs the sub-segments of a query edge"):
        polygons_in_polygons(off, xy, off, xy, predicate="contains")
    with pytest.raises(ValueError, match="neither 'contains' nor 'intersects'"):
        polygons_in_polygons(off, xy, off, xy, predicate="within")
    for bad in ("small", 0, "LARGE"):
        with pytest.raises(ValueError, match="_route"):
            polygon_overlaps(off, xy, off, xy, _route=bad)
    for bad in (0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="cells_per_polygon"):
            polygon_overlaps(off, xy, off, xy, cells_per_polygon=bad)
    with pytest.raises(ValueError, match="set A: ring_offsets"):
        polygon_overlaps(off.float(), xy, off, xy)
    with pytest.raises(ValueError, match="set B: xy"):
        polygon_overlaps(off, xy, off, xy[:, :1])
    with pytest.raises(ValueError, match="set B: ring_offsets and xy are tensors"):
        polygon_overlaps(off, xy, off.numpy(), xy)
    long_off, long_xy = (torch.from_numpy(t) for t in oc.csr([oc.SQUARE, oc.star(oc.MAX_VERTS + 1, 5, scale=1 << 20)]))
    with pytest.raises(ValueError, match="set B: polygon 1 has 4097 vertices"):
        polygon_overlaps(off, xy, long_off, long_xy)
    with pytest.raises(ValueError, match="set A: polygon 1 has 4097 vertices"):
        polygons_in_polygons(long_off, long_xy, off, xy)
    for fn in (lambda: polygon_overlaps(off, xy, off, xy), lambda: polygons_in_polygons(off, xy, off, xy)):
        with pytest.raises(_lib.SeggerAmdError, match="MI355X only"):
            fn()
    with pytest.raises(ValueError, match="the dict polygon_overlaps returns"):
        match_polygons({"pairs": torch.zeros(3, 2, dtype=torch.int64), "area": torch.zeros(2), "area_a": torch.zeros(1), "area_b": torch.zeros(1)})
    tie = {"pairs": torch.tensor([[0, 0, 1], [0, 1, 1]]), "area": torch.tensor([2.0, 2.0, 2.0], dtype=torch.float64),
           "area_a": torch.tensor([4.0, 4.0], dtype=torch.float64), "area_b": torch.tensor([4.0, 4.0, 1.0], dtype=torch.float64)}
    m = match_polygons(tie)                                          # plain torch: it runs wherever its input lives
    assert m["best_b"].tolist() == [0, 1] and m["best_a"].tolist() == [0, 0, -1] and m["n_overlapping_b"].tolist() == [1, 2, 0]
