"""The oracles and the case lists of the points-in-buffered-polygons tests (plain numpy and the standard library: no
product import).

The predicate, for a point t, a ring P (without its closing duplicate vertex) and a distance d >= 0:

    parity(t, P)  crossing number, half-open rule: an edge (a, b) counts when a.y <= t.y < b.y or b.y <= t.y < a.y and
                  the crossing lies strictly to the right of t
    dist2(t, P)   the smallest squared distance from t to a closed edge segment
    contains      dist2 < d*d or (parity and dist2 > 0)
    intersects    dist2 <= d*d or parity
    a ring of fewer than 3 vertices matches nothing

Two oracles:

* ``match_f64``: float64 on coordinates translated to the ring's first vertex, one ring against many points;
* ``pair_exact``: integers / ``fractions.Fraction`` (every coordinate of every case is a multiple of 2^-11, so the integers
  are what the float64 input holds); ``d*d`` is the float64 product the wrapper's kernel computes, taken exactly.

A pair is UNDECIDED when the exact oracle has it within the band of the decision boundary: ``d > 0``, the parity is false
(with the parity true and dist2 > 0 the point is in under both predicates whatever d is) and
``|dist2 - d*d| <= BAND * d*d``.  With ``d == 0`` nothing is undecided: the boundary is then ``dist2 == 0`` and the parity,
which float64 gets exactly on these coordinates (the cross product of translated multiples of 2^-11 is exact), and the
tests rely on on-ring points being decided.  ``BAND`` is ``8 x E_REF`` with a floor of 4 float64 ulp, ``E_REF`` the float64
oracle's largest relative error in dist2 against the exact one as tests/test_polygon_join_oracle.py measured it (it
asserts that the measurement does not exceed the record).  Undecided pairs are left out of comparisons and may be at most
``MAX_UNDECIDED`` of the oracle's pairs.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import morphology_cases as mc

SCALE = 2048                        # coordinates are multiples of 1 / SCALE (rings: of 1 / 1024; midpoints need one bit more)
ORIGIN = np.array([30000.25, 90000.5])
ULP = 2.0 ** -52
D_CASES = (0.0, 0.25)
PREDICATES = ("contains", "intersects")
MAX_UNDECIDED = 1e-3

# measured by test_polygon_join_oracle.py::test_float64_oracle_dist2_error (largest over the cases and the batch's sample)
E_REF = 1.1e-16
BAND = max(8.0 * E_REF, 4.0 * ULP)
# the batch is too large for the exact oracle pair by pair: it decides the pairs that float64 puts within NEAR (relative)
# of the boundary -- a million times the float64 oracle's error -- and a random sample of the others
NEAR = 1e-9


# ---------------------------------------------------------------- float64 oracle ---
def match_f64(points: np.ndarray, ring: np.ndarray, d: float) -> tuple:
    """one ring against points [N, 2] -> (contains [N] bool, intersects [N] bool, dist2 [N], parity [N] bool)"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    ring = mc.open_ring(ring)
    n_pts = len(points)
    if len(ring) < 3:
        no = np.zeros(n_pts, dtype=bool)
        return no, no.copy(), np.full(n_pts, np.inf), no.copy()
    v = ring - ring[0]
    p = points - ring[0]
    ax, ay = v[:, 0][None, :], v[:, 1][None, :]
    bx, by = np.roll(v[:, 0], -1)[None, :], np.roll(v[:, 1], -1)[None, :]
    px, py = p[:, 0][:, None], p[:, 1][:, None]
    ex, ey = bx - ax, by - ay
    wx, wy = px - ax, py - ay
    cr = ex * wy - ey * wx
    dot = wx * ex + wy * ey
    len2 = ex * ex + ey * ey
    a_below, b_below = ay <= py, by <= py
    crossing = (a_below & ~b_below & (cr > 0.0)) | (~a_below & b_below & (cr < 0.0))
    parity = (crossing.sum(axis=1) & 1).astype(bool)
    ux, uy = px - bx, py - by
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.where((dot <= 0.0) | (len2 == 0.0), wx * wx + wy * wy, np.where(dot >= len2, ux * ux + uy * uy, cr * cr / len2))
    dist2 = d2.min(axis=1)
    dd = np.float64(d) * np.float64(d)
    return (dist2 < dd) | (parity & (dist2 > 0.0)), (dist2 <= dd) | parity, dist2, parity


# ---------------------------------------------------------------- exact oracle ---
def _ints(a) -> list:
    out = []
    for x, y in np.asarray(a, dtype=np.float64).reshape(-1, 2):
        xi, yi = x * SCALE, y * SCALE
        assert xi == int(xi) and yi == int(yi), "a coordinate is no multiple of 1 / SCALE"
        out.append((int(xi), int(yi)))
    return out


def pair_exact(t: tuple, ring: list) -> tuple:
    """one point and one ring, both as integers (coordinates x SCALE) -> (parity, dist2 as a Fraction in true units), or
    (False, None) for a ring of fewer than 3 vertices"""
    n = len(ring)
    if n < 3:
        return False, None
    crossings = 0
    best_n, best_d = None, 1
    for j in range(n):
        (ax, ay), (bx, by) = ring[j], ring[(j + 1) % n]
        ex, ey, wx, wy = bx - ax, by - ay, t[0] - ax, t[1] - ay
        cr = ex * wy - ey * wx
        if (ay <= t[1] < by and cr > 0) or (by <= t[1] < ay and cr < 0):
            crossings += 1
        dot, len2 = wx * ex + wy * ey, ex * ex + ey * ey
        if dot <= 0 or len2 == 0:
            num, den = wx * wx + wy * wy, 1
        elif dot >= len2:
            num, den = (t[0] - bx) ** 2 + (t[1] - by) ** 2, 1
        else:
            num, den = cr * cr, len2
        if best_n is None or num * best_d < best_n * den:
            best_n, best_d = num, den
    return bool(crossings & 1), Fraction(best_n, best_d * SCALE * SCALE)


def decide_exact(parity: bool, dist2, d: float) -> tuple:
    """(contains, intersects, undecided) of one pair from the exact parity and dist2"""
    if dist2 is None:
        return False, False, False
    dd = Fraction(float(np.float64(d) * np.float64(d)))
    undecided = dd > 0 and not parity and abs(dist2 - dd) <= Fraction(BAND) * dd
    return dist2 < dd or (parity and dist2 > 0), dist2 <= dd or parity, undecided


# ---------------------------------------------------------------- many rings ---
def _bounds(rings) -> np.ndarray:
    out = np.full((len(rings), 4), np.nan)
    for p, r in enumerate(rings):
        r = mc.open_ring(r)
        if len(r):
            out[p] = (r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max())
    return out


def _candidates(points: np.ndarray, bounds: np.ndarray, p: int, d: float) -> np.ndarray:
    """the points within the bounds of ring p grown by d + 1: every other point is farther than d from the ring and
    outside it (these comparisons are exact)"""
    if np.isnan(bounds[p, 0]):
        return np.zeros(0, dtype=np.int64)
    g = d + 1.0
    return np.flatnonzero((points[:, 0] >= bounds[p, 0] - g) & (points[:, 0] <= bounds[p, 2] + g) &
                          (points[:, 1] >= bounds[p, 1] - g) & (points[:, 1] <= bounds[p, 3] + g))


def _pairs(rows) -> np.ndarray:
    a = np.asarray(sorted(rows), dtype=np.int64).reshape(-1, 2)
    return a


def join_f64(points, rings, dists) -> dict:
    """float64 oracle of the whole join -> {"contains": pairs, "intersects": pairs, "near": pairs}: int64 [E, 2] arrays of
    (point, polygon) sorted by (point, polygon); "near" holds the pairs with a false parity, d > 0 and dist2 within NEAR of
    d*d, the only ones that can be undecided"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    bounds = _bounds(rings)
    out = {"contains": [], "intersects": [], "near": []}
    for p, ring in enumerate(rings):
        d = float(dists[p])
        idx = _candidates(points, bounds, p, d)
        if len(idx) == 0:
            continue
        con, inter, dist2, parity = match_f64(points[idx], ring, d)
        dd = d * d
        near = (dd > 0) & ~parity & (np.abs(dist2 - dd) <= NEAR * dd)
        for name, mask in (("contains", con), ("intersects", inter), ("near", near)):
            out[name].append(np.stack([idx[mask], np.full(int(mask.sum()), p, dtype=np.int64)], axis=1))
    res = {}
    for name, parts in out.items():
        a = np.concatenate(parts + [np.zeros((0, 2), dtype=np.int64)]).astype(np.int64)
        res[name] = a[np.lexsort((a[:, 1], a[:, 0]))]
    return res


def join_exact(points, rings, dists, only=None) -> dict:
    """exact oracle -> {"contains": pairs, "intersects": pairs, "undecided": pairs, "dist2": {(point, polygon): Fraction}}
    over the bounding-box candidates of every ring, or over the (point, polygon) pairs of ``only``"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    ipts = _ints(points)
    irings = [_ints(mc.open_ring(r)) for r in rings]
    bounds = _bounds(rings)
    if only is None:
        todo = [(int(i), p) for p in range(len(rings)) for i in _candidates(points, bounds, p, float(dists[p]))]
    else:
        todo = [(int(i), int(p)) for i, p in only]
    out = {"contains": [], "intersects": [], "undecided": []}
    dist2 = {}
    for i, p in todo:
        parity, d2 = pair_exact(ipts[i], irings[p])
        con, inter, und = decide_exact(parity, d2, float(dists[p]))
        dist2[(i, p)] = d2
        for name, flag in (("contains", con), ("intersects", inter), ("undecided", und)):
            if flag:
                out[name].append((i, p))
    res = {name: _pairs(rows) for name, rows in out.items()}
    res["dist2"] = dist2
    return res


def without(pairs: np.ndarray, drop: np.ndarray) -> np.ndarray:
    """pairs [E, 2] without the rows of drop"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(drop) == 0:
        return pairs
    gone = {(int(a), int(b)) for a, b in drop}
    keep = np.fromiter(((int(a), int(b)) not in gone for a, b in pairs), dtype=bool, count=len(pairs))
    return pairs[keep]


# ---------------------------------------------------------------- the named cases ---
def _ring_cases() -> list:
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    star5 = np.array([[(5.0 if k % 2 == 0 else 2.0) * math.cos(math.pi / 2 + k * math.pi / 5),
                       (5.0 if k % 2 == 0 else 2.0) * math.sin(math.pi / 2 + k * math.pi / 5)] for k in range(10)])
    named = [
        ("square", sq),
        ("l_shape", np.array([[0.0, 0.0], [3.0, 0.0], [3.0, 1.0], [1.0, 1.0], [1.0, 3.0], [0.0, 3.0]])),
        ("star5", mc.quantize(star5)),
        ("regular13", mc.regular(13)),
        ("regular25", mc.regular(25)),
        ("star63", mc.star_ring(63, 63)),
        ("star64", mc.star_ring(64, 64)),
        ("star65", mc.star_ring(65, 65)),
        ("star200", mc.star_ring(200, 200)),
        ("square_closed", np.concatenate([sq, sq[:1]])),
    ]
    named += [(name + "_cw", ring[::-1].copy()) for name, ring in named]
    named += [
        ("empty", np.zeros((0, 2))),
        ("point", np.array([[2.5, 1.25]])),
        ("segment", np.array([[0.0, 0.0], [3.0, 4.0]])),
        ("collinear4", np.array([[0.0, 0.0], [2.0, 1.0], [1.0, 0.5], [4.0, 2.0]])),
    ]
    return named


def _point_cases(name: str, ring: np.ndarray) -> list:
    """(label, point) around one ring, in the ring's own coordinates; every point a multiple of 2^-11"""
    r = mc.open_ring(ring)
    eps = 2.0 ** -10
    if len(r) == 0:
        return [("origin", np.array([0.0, 0.0]))]
    pts = []
    n = len(r)
    lo, hi = r.min(0), r.max(0)
    for k in sorted({0, n // 3, n - 1}):
        pts.append((f"vertex{k}", r[k]))
    for k in sorted({0, n // 2}):
        a, b = r[k], r[(k + 1) % n]
        mid = (a + b) / 2
        pts.append((f"edge{k}_mid", mid))
        for dx, dy in ((eps, 0.0), (-eps, 0.0), (0.0, eps), (0.0, -eps)):
            pts.append((f"edge{k}_mid{dx:+g}{dy:+g}", mid + np.array([dx, dy])))
        e = b - a
        length = math.hypot(e[0], e[1])
        if length > 0:                                                # both sides of the edge: one of them is outside
            nrm = np.array([e[1], -e[0]]) / length
            for d in D_CASES[1:]:
                for f in (0.5, 2.0):
                    for s in (1.0, -1.0):
                        pts.append((f"edge{k}_{f}d{s:+g}", np.round((mid + s * f * d * nrm) * 1024) / 1024))
    for k in sorted({int(np.argmin(r[:, 1])), int(np.argmax(r[:, 1])), 0, n // 2}):    # the ray through a vertex
        pts.append((f"ray{k}_left", np.array([lo[0] - 3.0, r[k, 1]])))
        pts.append((f"ray{k}_right", np.array([hi[0] + 3.0, r[k, 1]])))
        pts.append((f"ray{k}_mid", np.array([(lo[0] + hi[0]) / 2, r[k, 1]])))
    c = int(np.lexsort((r[:, 1], r[:, 0]))[0])                       # the lowest (x, y) vertex: a convex corner
    for d in D_CASES[1:]:
        for f in (0.5, 2.0):
            pts.append((f"corner_{f}d_left", r[c] + np.array([-f * d, 0.0])))
            diag = f * d / math.sqrt(2.0)
            pts.append((f"corner_{f}d_diag", np.round((r[c] + np.array([-diag, -diag * (1 if r[c, 1] <= (lo[1] + hi[1]) / 2 else -1)])) * 1024) / 1024))
    pts.append(("centre", np.round((lo + hi) / 2 * 1024) / 1024))
    if name.startswith("l_shape"):
        pts.append(("notch", np.array([2.0, 2.0])))
        pts.append(("notch_corner", np.array([1.0, 1.0])))
        pts.append(("notch_near", np.array([1.0 + eps, 1.0 + eps])))
    return [(label, np.asarray(p, dtype=np.float64)) for label, p in pts]


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    """(rings, names, points, labels, owner): ring k sits at ORIGIN + (40 k, 0); ``points`` concatenates every ring's point
    cases (``owner[i]`` = the ring that point i was made for) and ends with one point far outside everything"""
    rings, names, points, labels, owner = [], [], [], [], []
    for k, (name, ring) in enumerate(_ring_cases()):
        shift = ORIGIN + np.array([40.0 * k, 0.0])
        rings.append(np.ascontiguousarray(ring + shift) if len(ring) else ring)
        names.append(name)
        for label, p in _point_cases(name, ring):
            points.append(p + shift)
            labels.append(f"{name}:{label}")
            owner.append(k)
    points.append(ORIGIN + np.array([-5000.0, 7000.0]))
    labels.append("far")
    owner.append(-1)
    return tuple(rings), tuple(names), np.asarray(points, dtype=np.float64), tuple(labels), np.asarray(owner)


# ---------------------------------------------------------------- the batch ---
BATCH_RATIOS = (0.0, 0.05)


@functools.lru_cache(maxsize=None)
def batch(seed: int = 11) -> tuple:
    """(rings, points): about 2 000 polygons on a 300 um field with about 50 000 points -- 13- and 25-vertex star rings about
    10 um across on a jittered 6.7 um lattice (they overlap their neighbours: many points belong to 3 or more), about 30
    rings of 65 .. 400 vertices, two of 64 and two of 65 vertices, either orientation, some closed, a few degenerate, and
    five rings off the field that no point reaches"""
    rng = np.random.default_rng(seed)
    side, per_row = 300.0, 45
    rings = []
    for p in range(per_row * per_row):
        gx, gy = p % per_row, p // per_row
        centre = (np.array([gx, gy]) + 0.5) * (side / per_row) + rng.uniform(-2.0, 2.0, 2)
        n = 13 if rng.uniform() < 0.6 else 25
        if p % 70 == 5:
            n = int(rng.integers(65, 401))
        if p in (100, 900):
            n = 64
        if p in (101, 901):
            n = 65
        ring = mc.star_ring(n, 20_000 + p, float(rng.uniform(4.0, 6.5)))
        if rng.uniform() < 0.5:
            ring = ring[::-1]
        if rng.uniform() < 0.3:
            ring = np.concatenate([ring, ring[:1]])
        if p % 401 == 7:
            ring = [np.zeros((0, 2)), np.array([[0.5, 0.5]]), np.array([[0.0, 0.0], [1.0, 1.0]])][(p // 401) % 3]
        rings.append(np.ascontiguousarray(ring + mc.quantize(ORIGIN + centre)) if len(ring) else ring)
    for k in range(5):
        rings.append(mc.star_ring(13, 30_000 + k, 5.0) + mc.quantize(ORIGIN + np.array([side + 30.0, 40.0 * k])))
    pts = mc.quantize(ORIGIN + rng.uniform(0.0, side, (50_000, 2)))
    on_ring = [rings[p][0] for p in range(3, 2000, 37) if len(rings[p]) >= 3]         # some points on a vertex
    return tuple(rings), np.concatenate([pts, np.asarray(on_ring)])


def batch_dists(ratio: float) -> np.ndarray:
    """sqrt(area / pi) * ratio of every ring of the batch (float64; the shoelace sum of these coordinates is exact); 0 for
    an empty ring"""
    rings, _ = batch()
    area = np.array([mc.props_f64(r)["area"] for r in rings])
    return np.where(np.isnan(area), 0.0, np.sqrt(area / math.pi) * ratio)


@functools.lru_cache(maxsize=None)
def reference(which: str, d_or_ratio: float) -> dict:
    """computed once per process.  ``"cases"`` at a distance d: the float64 join, the exact join over the bounding-box
    candidates.  ``"batch"`` at a ratio: the float64 join and the exact decision of its near-boundary pairs.
    -> {"f64": ..., "exact": ..., "undecided": pairs, "dists": [P]}"""
    if which == "cases":
        rings, _, points, _, _ = cases()
        dists = np.full(len(rings), float(d_or_ratio))
        f64 = join_f64(points, rings, dists)
        exact = join_exact(points, rings, dists)
    else:
        rings, points = batch()
        dists = batch_dists(float(d_or_ratio))
        f64 = join_f64(points, rings, dists)
        exact = join_exact(points, rings, dists, only=f64["near"])
    return {"f64": f64, "exact": exact, "undecided": exact["undecided"], "dists": dists}


def to_csr(rings) -> tuple:
    return mc.to_csr(rings)
