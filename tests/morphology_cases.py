"""The oracle and the case list of the boundary morphology tests (plain numpy and the standard library: no product
import).

Two oracles, one polygon at a time, both on the ring without its closing duplicate vertex:

* ``props_f64``: float64 on coordinates translated to the ring's first vertex -- shoelace, Andrew's monotone chain,
  rotating calipers as "every hull edge against every hull vertex", Welzl's iteration;
* ``props_exact``: the same quantities as ``fractions.Fraction`` from integer coordinates (every coordinate of every case
  is a multiple of 2^-10, so the integers are what the float64 input holds): ``area``, ``hull_area``, ``envelope_area``,
  ``rect_area`` = extent_u extent_v / |e|^2 and ``radius2`` (two support points: |d|^2 / 4; three: the squared
  circumradius), with exact predicates for hull membership, for the edge that wins and for the support set.

``E_REF`` is the largest relative deviation of ``props_f64`` from ``props_exact`` over every polygon below, per column,
as tests/test_morphology_oracle.py measured it (it asserts that the measurement does not exceed the record): the
yardstick of the device test, which allows 8 x E_REF with a floor of 4 float64 ulp.
"""
import functools
import math
from fractions import Fraction

import numpy as np

MAX_VERTS = 4096                    # SEGGER_MORPH_MAX_VERTS
SCALE = 1024                        # coordinates are multiples of 1 / SCALE
SLIDE = np.array([73211.25, 48907.5])
CIRCLE_SLACK = 2.0 ** -44           # SEGGER_MORPH_CIRCLE_SLACK
FLOAT_COLS = ("area", "hull_area", "rect_area", "envelope_area", "radius")
ULP = 2.0 ** -52

# measured by test_morphology_oracle.py::test_float64_oracle_agrees_with_exact (largest over all polygons below)
E_REF = {"area": 0.0, "hull_area": 0.0, "rect_area": 2.3e-16, "envelope_area": 0.0, "radius": 2.5e-16}


def tolerance(col: str) -> float:
    """relative tolerance of the device test for a column: 8 x E_REF, at least 4 ulp"""
    return max(8.0 * E_REF[col], 4.0 * ULP)


def quantize(a) -> np.ndarray:
    return np.round(np.asarray(a, dtype=np.float64) * SCALE) / SCALE


def open_ring(ring: np.ndarray) -> np.ndarray:
    """the ring without a closing duplicate of its first vertex (bit for bit)"""
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    if len(ring) >= 2 and ring[0].tobytes() == ring[-1].tobytes():
        return ring[:-1]
    return ring


# ---------------------------------------------------------------- float64 oracle ---
def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _hull_indices(pts) -> list:
    """Andrew's monotone chain -> indices of the strict hull vertices, counter-clockwise from the lowest (x, y); of equal
    points the lowest index.  ``pts`` is a sequence of (x, y) of floats or ints: the predicate is exact for ints."""
    order = sorted(range(len(pts)), key=lambda i: (pts[i][0], pts[i][1], i))
    uniq = [i for k, i in enumerate(order) if k == 0 or tuple(pts[i]) != tuple(pts[order[k - 1]])]
    if len(uniq) <= 2:
        return uniq
    lower, upper = [], []
    for chain, seq in ((lower, uniq), (upper, uniq[::-1])):
        for i in seq:
            while len(chain) >= 2 and _cross(pts[chain[-2]], pts[chain[-1]], pts[i]) <= 0:
                chain.pop()
            chain.append(i)
    return lower[:-1] + upper[:-1]


def _circle2(a, b):
    cx, cy = a[0] + (b[0] - a[0]) / 2, a[1] + (b[1] - a[1]) / 2
    return cx, cy, max(_d2(a, cx, cy), _d2(b, cx, cy))


def _circle3(a, b, c):
    bx, by, cx, cy = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
    d = 2 * (bx * cy - by * cx)
    b2, c2 = bx * bx + by * by, cx * cx + cy * cy
    ox, oy = a[0] + (cy * b2 - by * c2) / d, a[1] + (bx * c2 - cx * b2) / d
    return ox, oy, max(_d2(a, ox, oy), _d2(b, ox, oy), _d2(c, ox, oy))


def _d2(p, cx, cy):
    return (p[0] - cx) * (p[0] - cx) + (p[1] - cy) * (p[1] - cy)


def _welzl(pts, slack):
    """smallest enclosing circle of pts (distinct, not all collinear unless <= 2) -> (cx, cy, r2); works on floats (with a
    relative slack on the containment test) and on Fractions (slack 0: exact)"""
    def outside(p, c):
        return _d2(p, c[0], c[1]) > c[2] + c[2] * slack
    c = (pts[0][0], pts[0][1], 0 * pts[0][0])
    for i in range(1, len(pts)):
        if not outside(pts[i], c):
            continue
        c = (pts[i][0], pts[i][1], 0 * pts[0][0])
        for j in range(i):
            if not outside(pts[j], c):
                continue
            c = _circle2(pts[i], pts[j])
            for k in range(j):
                if outside(pts[k], c):
                    c = _circle3(pts[i], pts[j], pts[k])
    return c


def props_f64(ring) -> dict:
    """float64 oracle of one ring -> area, hull_area, rect_area, envelope_area, radius, centroid, bounds, n_hull, hull"""
    ring = open_ring(ring)
    n = len(ring)
    nan = float("nan")
    if n == 0:
        return dict(area=nan, hull_area=nan, rect_area=nan, envelope_area=nan, radius=nan, centroid=(nan, nan),
                    bounds=(nan,) * 4, n_hull=0, hull=[])
    t = ring - ring[0]
    x, y = t[:, 0], t[:, 1]
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    cr = x * yn - xn * y
    a2 = float(cr.sum())
    if a2 != 0.0:
        centroid = (ring[0, 0] + float(((x + xn) * cr).sum()) / (3 * a2), ring[0, 1] + float(((y + yn) * cr).sum()) / (3 * a2))
    else:
        centroid = (ring[0, 0] + float(x.sum()) / n, ring[0, 1] + float(y.sum()) / n)
    bounds = (ring[:, 0].min(), ring[:, 1].min(), ring[:, 0].max(), ring[:, 1].max())
    hull = _hull_indices([(float(p[0]), float(p[1])) for p in t])
    hp = t[hull]
    h = len(hull)
    hx, hy = hp[:, 0], hp[:, 1]
    hull_area = 0.5 * abs(float((hx * np.roll(hy, -1) - np.roll(hx, -1) * hy).sum()))
    rect = 0.0
    if h >= 2:
        e = np.roll(hp, -1, axis=0) - hp                              # [h, 2]
        d = hp[None, :, :] - hp[:, None, :]                           # d[k, j] = hull vertex j - start of edge k
        u = d[:, :, 0] * e[:, None, 0] + d[:, :, 1] * e[:, None, 1]
        v = d[:, :, 1] * e[:, None, 0] - d[:, :, 0] * e[:, None, 1]
        areas = (u.max(1) - u.min(1)) * (v.max(1) - v.min(1)) / (e[:, 0] ** 2 + e[:, 1] ** 2)
        rect = float(areas.min())
    c = _welzl([(float(p[0]), float(p[1])) for p in hp], CIRCLE_SLACK)
    return dict(area=0.5 * abs(a2), hull_area=hull_area, rect_area=rect,
                envelope_area=float((bounds[2] - bounds[0]) * (bounds[3] - bounds[1])), radius=math.sqrt(c[2]), centroid=centroid,
                bounds=bounds, n_hull=h, hull=hull)


# ---------------------------------------------------------------- exact oracle ---
def props_exact(ring) -> dict:
    """exact oracle of one ring (coordinates multiples of 1 / SCALE) -> Fractions area, hull_area, rect_area,
    envelope_area, radius2; n_hull, hull (indices), rect_edge (index of the first hull edge that attains the minimum).
    An empty ring -> None for every quantity."""
    ring = open_ring(ring)
    n = len(ring)
    if n == 0:
        return dict(area=None, hull_area=None, rect_area=None, envelope_area=None, radius2=None, n_hull=0, hull=[])
    pts = []
    for p in ring:
        xi, yi = p[0] * SCALE, p[1] * SCALE
        assert xi == int(xi) and yi == int(yi), "a coordinate is no multiple of 1 / SCALE"
        pts.append((int(xi), int(yi)))
    s2 = SCALE * SCALE

    def shoelace2(idx):
        return abs(sum(pts[a][0] * pts[b][1] - pts[b][0] * pts[a][1] for a, b in zip(idx, idx[1:] + idx[:1])))
    hull = _hull_indices(pts)
    h = len(hull)
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    rect, rect_edge = Fraction(0), 0
    if h >= 2:
        best = None
        for k in range(h):
            a, b = pts[hull[k]], pts[hull[(k + 1) % h]]
            ex, ey = b[0] - a[0], b[1] - a[1]
            u = [(pts[j][0] - a[0]) * ex + (pts[j][1] - a[1]) * ey for j in hull]
            v = [(pts[j][1] - a[1]) * ex - (pts[j][0] - a[0]) * ey for j in hull]
            area = Fraction((max(u) - min(u)) * (max(v) - min(v)), ex * ex + ey * ey)
            if best is None or area < best:
                best, rect_edge = area, k
        rect = best / s2
    c = _welzl([(Fraction(pts[j][0]), Fraction(pts[j][1])) for j in hull], 0)
    return dict(area=Fraction(shoelace2(list(range(n))), 2 * s2), hull_area=Fraction(shoelace2(hull), 2 * s2), rect_area=rect,
                envelope_area=Fraction((max(xs) - min(xs)) * (max(ys) - min(ys)), s2), radius2=Fraction(c[2]) / s2, n_hull=h,
                hull=hull, rect_edge=rect_edge)


def exact_floats(ex: dict) -> dict:
    """the five float quantities of an exact result, each rounded once (radius: a correctly rounded quotient, then sqrt)"""
    if ex["area"] is None:
        return {c: float("nan") for c in FLOAT_COLS}
    out = {c: ex[c].numerator / ex[c].denominator for c in FLOAT_COLS if c != "radius"}
    out["radius"] = math.sqrt(ex["radius2"].numerator / ex["radius2"].denominator)
    return out


def scipy_area_tolerance(pts: np.ndarray) -> float:
    """absolute error allowed to scipy's hull area: Qhull sums products of the UNTRANSLATED coordinates, each up to
    max|x| max|y| and rounded to an ulp of that; 64 such roundings cover the facets of every case here"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    return 64.0 * ULP * max(float(np.abs(pts[:, 0]).max()) * float(np.abs(pts[:, 1]).max()), 1.0)


def rel_dev(got: float, want: float) -> float:
    if want == 0.0:
        return 0.0 if got == 0.0 else math.inf
    return abs(got - want) / abs(want)


# ---------------------------------------------------------------- the cases ---
def star_ring(n: int, seed: int, radius: float = 8.0) -> np.ndarray:
    """a random star-shaped ring of n vertices around the origin, counter-clockwise, quantised"""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, 2 * np.pi, n))
    r = radius * rng.uniform(0.4, 1.0, n)
    return quantize(np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1))


def regular(n: int, radius: float = 6.0) -> np.ndarray:
    ang = 2 * np.pi * np.arange(n) / n
    return quantize(np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1))


def _named() -> list:
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    c30, s30 = math.cos(math.pi / 6), math.sin(math.pi / 6)
    rect = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 1.0], [0.0, 1.0]]) @ np.array([[c30, s30], [-s30, c30]])
    star5 = np.array([[(5.0 if k % 2 == 0 else 2.0) * math.cos(math.pi / 2 + k * math.pi / 5),
                       (5.0 if k % 2 == 0 else 2.0) * math.sin(math.pi / 2 + k * math.pi / 5)] for k in range(10)])
    cases = [
        ("triangle", [[0, 0], [4, 0], [1, 3]]),
        ("square_ccw", sq),
        ("square_cw", sq[::-1]),
        ("square_closed", np.concatenate([sq, sq[:1]])),
        ("square_edge_vertices", [[0, 0], [0.25, 0], [0.5, 0], [1, 0], [1, 0.5], [1, 1], [0.75, 1], [0, 1], [0, 0.5]]),
        ("square_repeated", [[0, 0], [0, 0], [1, 0], [1, 0], [1, 0], [1, 1], [0, 1], [0, 1]]),
        ("l_shape", [[0, 0], [3, 0], [3, 1], [1, 1], [1, 3], [0, 3]]),
        ("star5", quantize(star5)),
        ("rect_10x1_rot30", quantize(rect)),
        ("acute", [[0, 0], [4, 0], [2.5, 3.5]]),
        ("obtuse", [[0, 0], [6, 0], [1, 1]]),
        ("regular13", regular(13)),
        ("regular25", regular(25)),
        ("star63", star_ring(63, 63)),
        ("star64", star_ring(64, 64)),
        ("star65", star_ring(65, 65)),
        ("star200", star_ring(200, 200)),
        ("star_max", star_ring(MAX_VERTS, 4096, 10.0)),
    ]
    return [(name, np.asarray(r, dtype=np.float64)) for name, r in cases]


def _degenerate() -> list:
    return [
        ("empty", np.zeros((0, 2))),
        ("point", np.array([[2.5, 1.25]])),
        ("segment", np.array([[0.0, 0.0], [3.0, 4.0]])),
        ("collinear5", np.array([[0.0, 0.0], [2.0, 1.0], [1.0, 0.5], [4.0, 2.0], [3.0, 1.5]])),
        ("identical", np.array([[1.5, 2.5]] * 4)),
    ]


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    """((name, ring), ...): the named cases, each again on slide coordinates, then the degenerate rings"""
    named = _named()
    return tuple(named + [(name + "_slide", ring + SLIDE) for name, ring in named] + _degenerate())


NON_DEGENERATE = tuple(name for name, _ in _named()) + tuple(name + "_slide" for name, _ in _named())
DEGENERATE = tuple(name for name, _ in _degenerate())


@functools.lru_cache(maxsize=None)
def batch(n_polygons: int = 1000, seed: int = 7) -> tuple:
    """n_polygons mixed rings on slide coordinates: mostly 3 .. 30 vertices, some around the route boundary, some long,
    either orientation, some closed, a few degenerate"""
    rng = np.random.default_rng(seed)
    rings = []
    for p in range(n_polygons):
        u = rng.uniform()
        n = int(rng.integers(3, 31)) if u < 0.88 else int(rng.integers(60, 70)) if u < 0.94 else int(rng.integers(100, 201))
        ring = star_ring(n, 10_000 + p, float(rng.uniform(3.0, 12.0)))
        if rng.uniform() < 0.5:
            ring = ring[::-1]
        if rng.uniform() < 0.3:
            ring = np.concatenate([ring, ring[:1]])
        if p % 97 == 0:
            ring = _degenerate()[(p // 97) % 5][1]
        rings.append(np.ascontiguousarray(ring + quantize(SLIDE + rng.uniform(-500.0, 500.0, 2))))
    return tuple(rings)


def to_csr(rings) -> tuple:
    """rings -> (ring_offsets int64 [P + 1], xy float64 [V, 2])"""
    offsets = np.zeros(len(rings) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rings])
    xy = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings] + [np.zeros((0, 2))])
    return offsets, xy


@functools.lru_cache(maxsize=None)
def reference(which: str = "cases") -> tuple:
    """(f64 results, exact results) of ``cases()`` or of ``batch()``, computed once per process"""
    rings = [r for _, r in cases()] if which == "cases" else list(batch())
    return tuple(props_f64(r) for r in rings), tuple(props_exact(r) for r in rings)


def ratios(area, hull_area, rect_area, envelope_area, radius):
    """the reference's four columns by numpy's division (x / 0 = +-inf, 0 / 0 = nan)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a, h, r, e, rad = (np.asarray(v, dtype=np.float64) for v in (area, hull_area, rect_area, envelope_area, radius))
        return np.stack([a, h / a, r / e, a / rad ** 2], axis=-1)
