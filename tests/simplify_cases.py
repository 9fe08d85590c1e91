"""CPU oracles and cases for segger_amd.simplify (numpy and fractions only; no GPU, no shapely).

* :func:`simplify_ring` -- the contract of include/segger_amd.h, sequential and recursive in float64: guarded Douglas-Peucker
  over the closed vertex sequence.  numpy evaluates the same IEEE operations in the same order as the kernel (no fused
  multiply-add), so the device result must be equal, not close.
* :func:`textbook_dp` -- the classical algorithm, written separately (a loop over a stack of open sections, scalar
  arithmetic), for ``preserve_topology=False``.
* :func:`shared_exact` / :func:`touch_exact` -- what two segments share, from the rational solution of the two parametric
  equations (with divisions; nothing in common with the kernel's orientation tests), and :func:`ring_simple_exact`, the
  simplicity of a ring with integer coordinates below 2^25, in int64 where every product is exact.
"""
import sys
from fractions import Fraction

import numpy as np

MAX_VERTS = 4096
SMALL_VERTS = 256
OK, TOO_FEW, TOUCH = 0, 1, 2
COUNTERS = ("n_vertices_in", "n_vertices_out", "n_sections", "n_refused", "n_passed_through", "n_restored", "longest_ring")


# ---------------------------------------------------------------- float64: the contract ---
def open_ring(ring):
    """the vertices of a ring without a closing duplicate (dropped bit for bit)"""
    pts = np.ascontiguousarray(np.asarray(ring, np.float64).reshape(-1, 2))
    if len(pts) >= 2 and pts[0].tobytes() == pts[-1].tobytes():
        pts = pts[:-1]
    return pts


def dist2_many(v, a, b):
    """squared distance from each row of v to the closed segment (a, b), csrc/polygon_join.hip's order of operations"""
    ex, ey = b[0] - a[0], b[1] - a[1]
    wx, wy = v[:, 0] - a[0], v[:, 1] - a[1]
    cr = ex * wy - ey * wx
    dot = wx * ex + wy * ey
    len2 = ex * ex + ey * ey
    ux, uy = v[:, 0] - b[0], v[:, 1] - b[1]
    with np.errstate(all="ignore"):
        return np.where((dot <= 0.0) | (len2 == 0.0), wx * wx + wy * wy, np.where(dot >= len2, ux * ux + uy * uy, cr * cr / len2))


def _orient_many(a, b, c):
    d = (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])
    return np.sign(d).astype(np.int64)


def _same(p, q):
    return (p[..., 0] == q[..., 0]) & (p[..., 1] == q[..., 1])


def _inside_of(o, p, q, r):
    box = (np.minimum(q[..., 0], r[..., 0]) <= p[..., 0]) & (p[..., 0] <= np.maximum(q[..., 0], r[..., 0])) & \
          (np.minimum(q[..., 1], r[..., 1]) <= p[..., 1]) & (p[..., 1] <= np.maximum(q[..., 1], r[..., 1]))
    return (o == 0) & box & ~_same(p, q) & ~_same(p, r)


def touch_many(a, b, c, d):
    """touch of the segment (a, b) with each segment (c[k], d[k]); float64 or int64 arrays alike"""
    a, b = np.broadcast_to(a, c.shape), np.broadcast_to(b, c.shape)
    o1, o2, o3, o4 = _orient_many(a, b, c), _orient_many(a, b, d), _orient_many(c, d, a), _orient_many(c, d, b)
    proper = (o1 * o2 < 0) & (o3 * o4 < 0)
    inside = _inside_of(o1, c, a, b) | _inside_of(o2, d, a, b) | _inside_of(o3, a, c, d) | _inside_of(o4, b, c, d)
    equal = ~_same(a, b) & ((_same(a, c) & _same(b, d)) | (_same(a, d) & _same(b, c)))
    return proper | inside | equal


def simplify_ring(ring, tol, preserve_topology=True):
    """-> (kept indices into the ring as given, stats): the contract, by recursion"""
    pts = open_ring(ring)
    n = len(pts)
    st = {"n_in": n, "sections": 0, "refused": 0, "kind": "", "max_pending": 0}
    if n < 3:
        st["kind"] = "passed"
        return list(range(n)), st
    v = pts - pts[0]
    v = np.vstack([v, v[:1]])                                         # index n is vertex 0
    tol2 = float(tol) * float(tol)
    kept = [0]

    def blocked(i, j):
        ks = list(range(0, i)) + list(range(j, n))
        s0 = np.array(ks + kept[:-1], np.int64)
        s1 = np.array([k + 1 for k in ks] + kept[1:], np.int64)
        return len(s0) > 0 and bool(touch_many(v[i], v[j], v[s0], v[s1]).any())

    def visit(i, j, pending):
        st["sections"] += 1
        st["max_pending"] = max(st["max_pending"], pending)
        if j > i + 1:
            d = dist2_many(v[i + 1:j], v[i], v[j])
            m = i + 1 + int(np.argmax(d))                            # the first of equal maxima
            flat = bool(d[m - i - 1] <= tol2)
            if flat and preserve_topology and blocked(i, j):
                st["refused"] += 1
                flat = False
            if not flat:
                visit(i, m, pending + 1)
                visit(m, j, pending)
                return
        if j < n:
            kept.append(j)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 3 * n + 1000))
    try:
        visit(0, n, 0)
    finally:
        sys.setrecursionlimit(limit)
    if len(kept) < 3:
        st["kind"] = "restored"
        kept = list(range(n))
    return kept, st


def _dist2(v, a, b):
    ex, ey = b[0] - a[0], b[1] - a[1]
    wx, wy = v[0] - a[0], v[1] - a[1]
    cr = ex * wy - ey * wx
    dot = wx * ex + wy * ey
    len2 = ex * ex + ey * ey
    if dot <= 0.0 or len2 == 0.0:
        return wx * wx + wy * wy
    if dot >= len2:
        ux, uy = v[0] - b[0], v[1] - b[1]
        return ux * ux + uy * uy
    return cr * cr / len2


def textbook_dp(ring, tol):
    """classical Douglas-Peucker of the closed sequence v0 .. v(n-1), v0 -> kept indices (all of them when fewer than 3 stay)"""
    pts = open_ring(ring)
    n = len(pts)
    if n < 3:
        return list(range(n))
    v = [(float(x - pts[0][0]), float(y - pts[0][1])) for x, y in pts]
    v.append(v[0])
    keep = [False] * (n + 1)
    keep[0] = keep[n] = True
    todo = [(0, n)]
    while todo:
        i, j = todo.pop()
        best, m = -1.0, -1
        for k in range(i + 1, j):
            d = _dist2(v[k], v[i], v[j])
            if d > best:
                best, m = d, k
        if m >= 0 and best > tol * tol:
            keep[m] = True
            todo += [(i, m), (m, j)]
    kept = [k for k in range(n) if keep[k]]
    return kept if len(kept) >= 3 else list(range(n))


# ---------------------------------------------------------------- exact: rationals and int64 ---
def shared_exact(a, b, c, d):
    """what the closed segments (a, b) and (c, d) share: None, ('point', X) or ('overlap',) -- rational arithmetic"""
    a, b, c, d = (tuple(Fraction(int(t)) for t in p) for p in (a, b, c, d))

    def sub(p, q):
        return (p[0] - q[0], p[1] - q[1])

    def cross(p, q):
        return p[0] * q[1] - p[1] * q[0]

    def dot(p, q):
        return p[0] * q[0] + p[1] * q[1]

    def point_on(p, q, r):                                           # p on the closed segment (q, r), q != r
        w, s = sub(p, q), sub(r, q)
        return cross(w, s) == 0 and 0 <= dot(w, s) <= dot(s, s)

    r, s = sub(b, a), sub(d, c)
    if r == (0, 0) and s == (0, 0):
        return ("point", a) if a == c else None
    if r == (0, 0):
        return ("point", a) if point_on(a, c, d) else None
    if s == (0, 0):
        return ("point", c) if point_on(c, a, b) else None
    qp = sub(c, a)
    rxs = cross(r, s)
    if rxs != 0:
        t, u = cross(qp, s) / rxs, cross(qp, r) / rxs
        if 0 <= t <= 1 and 0 <= u <= 1:
            return ("point", (a[0] + t * r[0], a[1] + t * r[1]))
        return None
    if cross(qp, r) != 0:
        return None
    t0 = dot(qp, r) / dot(r, r)
    t1 = t0 + dot(s, r) / dot(r, r)
    lo, hi = max(Fraction(0), min(t0, t1)), min(Fraction(1), max(t0, t1))
    if lo > hi:
        return None
    if lo == hi:
        return ("point", (a[0] + lo * r[0], a[1] + lo * r[1]))
    return ("overlap",)


def touch_exact(a, b, c, d):
    sh = shared_exact(a, b, c, d)
    if sh is None:
        return False
    if sh[0] == "overlap":
        return True
    x = sh[1]
    ends = lambda p, q: x == tuple(Fraction(int(t)) for t in p) or x == tuple(Fraction(int(t)) for t in q)
    return not (ends(a, b) and ends(c, d))


def as_grid(ring):
    pts = open_ring(ring)
    g = pts.astype(np.int64)
    assert np.array_equal(g.astype(np.float64), pts) and (np.abs(g) < (1 << 25)).all(), "grid coordinates below 2^25 only"
    return g


def ring_simple_exact(ring, fractions=False):
    """-> (ok, (code, i, j)) for a ring with integer coordinates; ``fractions``: every pair through touch_exact (slow)"""
    g = as_grid(ring)
    n = len(g)
    nxt = np.roll(g, -1, axis=0) if n else g
    if n < 3 or int((~_same(g, nxt)).sum()) < 3:
        return False, (TOO_FEW, -1, -1)
    for i in range(n - 1):
        if fractions:
            hit = np.array([touch_exact(g[i], nxt[i], g[j], nxt[j]) for j in range(i + 1, n)])
        else:
            hit = touch_many(g[i], nxt[i], g[i + 1:], nxt[i + 1:])
        if hit.any():
            return False, (TOUCH, i, i + 1 + int(np.argmax(hit)))
    return True, (OK, -1, -1)


# ---------------------------------------------------------------- batches ---
def csr(rings):
    rings = [np.asarray(r, np.float64).reshape(-1, 2) for r in rings]
    off = np.zeros(len(rings) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rings])
    xy = np.concatenate(rings) if rings else np.zeros((0, 2))
    return off, np.ascontiguousarray(xy, np.float64)


def expected(rings, tol, preserve_topology=True):
    """every tensor and counter simplify_rings returns for the CSR of ``rings``; tol: one value or one per ring"""
    off, xy = csr(rings)
    tols = np.broadcast_to(np.asarray(tol, np.float64), (len(rings),))
    out_off, idx = [0], []
    c = dict.fromkeys(COUNTERS, 0)
    for p, ring in enumerate(rings):
        kept, st = simplify_ring(ring, float(tols[p]), preserve_topology)
        idx += [int(off[p]) + k for k in kept]
        out_off.append(len(idx))
        c["n_vertices_in"] += st["n_in"]
        c["n_vertices_out"] += len(kept)
        c["n_sections"] += st["sections"]
        c["n_refused"] += st["refused"]
        c["n_passed_through"] += st["kind"] == "passed"
        c["n_restored"] += st["kind"] == "restored"
        c["longest_ring"] = max(c["longest_ring"], len(kept))
    idx = np.array(idx, np.int64)
    return {"ring_offsets": np.array(out_off, np.int64), "xy": xy[idx].reshape(-1, 2), "vertex_index": idx,
            "counters": np.array([c[k] for k in COUNTERS], np.int64)}


def expected_simple(rings):
    res = [ring_simple_exact(r) for r in rings]
    return np.array([r[0] for r in res], bool), np.array([r[1] for r in res], np.int32).reshape(-1, 3)


def area2(ring):
    """twice the signed area of an integer ring, exactly"""
    g = as_grid(ring)
    x, y = g[:, 0], g[:, 1]
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def contour_tolerance(rings, frac=1.0 / 50.0):
    return float(np.mean([np.sqrt(abs(area2(r)) / 2.0) for r in rings]) * frac)


# ---------------------------------------------------------------- cases ---
# the U of the first four vertices is within 2 of its chord y = 0; a peninsula of the opposite side reaches into it
U_CROSSED = [(0, 0), (5, -2), (15, -2), (20, 0), (20, 10), (11, 10), (10, -1), (9, 10), (0, 10)]
U_TIP_ON_CHORD = [(0, 0), (5, -2), (15, -2), (20, 0), (20, 10), (11, 10), (10, 0), (9, 10), (0, 10)]

HAND = {                                                             # name: (ring, tolerance)
    "square_midpoints": ([(0, 0), (2, 0), (4, 0), (4, 2), (4, 4), (2, 4), (0, 4), (0, 2)], 0.0),
    "tie_for_farthest": ([(0, 0), (3, 4), (5, 0), (3, -4)], 1.0),
    "u_crossed": (U_CROSSED, 2.0),
    "u_tip_on_chord": (U_TIP_ON_CHORD, 2.0),
    "flat_abcb": ([(0, 0), (2, 0), (4, 0), (2, 0)], 1.0),
    "all_equal": ([(1, 1)] * 5, 0.5),
    "consecutive_duplicates": ([(0, 0), (0, 0), (6, 0), (6, 0), (6, 0), (6, 5), (0, 5), (0, 5)], 0.5),
    "closing_duplicate": ([(3, 1), (9, 1), (9, 2), (9, 7), (3, 7), (3, 1)], 0.0),
    "neck_revisits_vertex": ([(0, 1), (1, 0), (2, 1), (3, 0), (4, 1), (3, 2), (2, 1), (1, 2)], 0.5),
    "n1": ([(7, 7)], 1.0),
    "n2": ([(7, 7), (8, 9)], 1.0),
    "n2_closed": ([(7, 7), (8, 9), (7, 7)], 1.0),
    "n3": ([(0, 0), (4, 0), (0, 3)], 1.0),
    "n0": ([], 1.0),
}
HAND_KEPT = {                                                        # worked by hand
    "square_midpoints": [0, 2, 4, 6], "flat_abcb": [0, 1, 2, 3], "all_equal": [0, 1, 2, 3], "n1": [0], "n2": [0, 1],
    "n2_closed": [0, 1], "n3": [0, 1, 2], "n0": [], "closing_duplicate": [0, 1, 3, 4], "tie_for_farthest": [0, 1, 2, 3],
}
BOUNDARY_SIZES = (3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096)


def star_ring(n, seed, r_lo=0.35, r_hi=1.0, scale=None):
    """a star-shaped ring of n integer vertices around the origin, ragged: the radius of each is drawn anew"""
    rng = np.random.default_rng(seed)
    scale = scale if scale is not None else max(40.0, 6.0 * n)
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
    rad = rng.uniform(r_lo, r_hi, n) * scale
    return np.stack([np.rint(rad * np.cos(ang)), np.rint(rad * np.sin(ang))], 1) + rng.integers(-1000, 1000, 2)


def comb_ring(n):
    """a square spiral growing by 2 % a vertex: of every section the LAST interior vertex is the farthest, so the splits are
    as unbalanced as they get and the pending right halves pile up to about n"""
    k = np.arange(n)
    r = 1.02 ** k
    return np.stack([r * np.cos(k * np.pi / 2.0), r * np.sin(k * np.pi / 2.0)], 1)


def boundary_rings():
    """(name, ring, tolerance): a ragged star at every size where the kernels change tier or chunk count, and the comb"""
    out = [(f"star_{n}", star_ring(n, 100 + n), 0.01 * max(40.0, 6.0 * n)) for n in BOUNDARY_SIZES]
    out += [(f"comb_{n}", comb_ring(n), 0.0) for n in (256, 257, 4096)]
    return out


_VORONOI = []


def voronoi_rings():
    """the rings tests/contour_cases.py's oracle yields on its small Voronoi scene (computed once)"""
    if not _VORONOI:
        import contour_cases as cc
        res = cc.label_rings(cc.voronoi_small())
        _VORONOI.extend(np.array(res[k]["ring"], np.float64) for k in sorted(res) if res[k]["ring"] is not None)
    return list(_VORONOI)


def random_rings():
    """ragged stars of 5 .. 300 vertices: coarse grids and deep notches, so that chords often run into the ring"""
    rng = np.random.default_rng(7)
    out = []
    for s in range(48):
        n = int(rng.integers(5, 300)) if s % 6 else int(rng.integers(250, 300))
        out.append(star_ring(n, 1000 + s, r_lo=0.15 if s % 2 else 0.5, scale=float(rng.integers(12, 90))))
    return out


TOLERANCES = (0.0, 0.5, 1.0, 2.0)
