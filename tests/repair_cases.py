"""CPU oracle and cases for segger_amd.repair (numpy and fractions only; no GPU, no shapely).

* :func:`centre` -- the centre of include/segger_amd.h in its stated order of summation (64 strided partial sums, six
  butterfly rounds, one addition of vertex 0, one division), so that its bits are the kernel's for any coordinates.
* :func:`resort_order` -- the contract, sequentially: the float64 differences from the centre are turned into
  ``fractions.Fraction`` and everything after that is exact -- the half-plane class, the sign of the cross product, the
  squared length; ties by input index.  The device result must be equal, not close.
* :func:`expected_resort` / :func:`expected_repair` -- every tensor ``resort_rings`` / ``repair_rings`` return for a list of
  rings; validity is tests/simplify_cases.py's exact integer oracle, so ``expected_repair`` takes grid rings only.
* the cases: rings at every size where the kernel changes its padded size, its chunk count or its tier; hand-worked tie
  rings; pairs that a float64 cross product or a float64 ``atan2`` key orders wrongly (asserted here, on the CPU).
"""
import functools
from fractions import Fraction

import numpy as np

import simplify_cases as sc

MAX_VERTS = 4096
SIZES = (3, 4, 5, 63, 64, 65, 100, 255, 256, 257, 300, 3000, 4096)
COUNTERS = ("n_invalid_in", "n_resorted", "n_still_invalid")
LANES = 64


# ---------------------------------------------------------------- the contract ---
def entries_of(ring):
    return np.ascontiguousarray(np.asarray(ring, np.float64).reshape(-1, 2))


def centre(pts):
    """(sum of the n open vertices + vertex 0) / (n + 1), summed in the header's order"""
    n = len(pts)
    part = np.zeros((LANES, 2))
    for base in range(0, n, LANES):                                  # lane l adds vertices l, l + 64, ... in ascending order
        chunk = pts[base:base + LANES]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    lanes = np.arange(LANES)
    for m in (1, 2, 4, 8, 16, 32):
        part = part + part[lanes ^ m]
    return (part[0] + pts[0]) / float(n + 1)


def differences(ring):
    """the rounded float64 differences of every entry of the ring (a closing duplicate included) from the centre"""
    ent = entries_of(ring)
    return ent - centre(sc.open_ring(ent))


def angle_class(dx, dy):
    """0: angle in (-pi, 0); 1: angle 0 (the zero vector too); 2: angle in (0, pi); 3: angle pi"""
    if dy < 0:
        return 0
    if dy > 0:
        return 2
    return 3 if dx < 0 else 1


def exact_compare(da, db, a=0, b=0):
    """-1 / 0 / 1: does the difference vector da come before db?  Exact: Fractions of the float64 values."""
    ax, ay, bx, by = (Fraction(float(t)) for t in (da[0], da[1], db[0], db[1]))
    ca, cb = angle_class(ax, ay), angle_class(bx, by)
    if ca != cb:
        return -1 if ca < cb else 1
    cross = ax * by - ay * bx
    if cross != 0:
        return -1 if cross > 0 else 1
    la, lb = ax * ax + ay * ay, bx * bx + by * by
    if la != lb:
        return -1 if la < lb else 1
    return (a > b) - (a < b)


def resort_order(ring):
    """the entries of the ring in the contract's order (indices into the ring as given)"""
    ent = entries_of(ring)
    if len(sc.open_ring(ent)) < 3:
        return list(range(len(ent)))
    d = differences(ent)
    f = [(Fraction(float(x)), Fraction(float(y))) for x, y in d]
    cls = [angle_class(x, y) for x, y in f]
    len2 = [x * x + y * y for x, y in f]

    def compare(a, b):
        if cls[a] != cls[b]:
            return -1 if cls[a] < cls[b] else 1
        cross = f[a][0] * f[b][1] - f[a][1] * f[b][0]
        if cross != 0:
            return -1 if cross > 0 else 1
        if len2[a] != len2[b]:
            return -1 if len2[a] < len2[b] else 1
        return a - b

    return sorted(range(len(ent)), key=functools.cmp_to_key(compare))


def expected_resort(rings, select=None):
    off, xy = sc.csr(rings)
    idx = []
    for p, ring in enumerate(rings):
        order = resort_order(ring) if select is None or select[p] else list(range(len(entries_of(ring))))
        idx += [int(off[p]) + k for k in order]
    idx = np.array(idx, np.int64)
    return {"xy": xy[idx].reshape(-1, 2), "vertex_index": idx}


def expected_repair(rings):
    """what repair_rings(on_failure='keep') returns for grid rings"""
    off, xy = sc.csr(rings)
    idx, status, before, after = [], [], [], []
    for p, ring in enumerate(rings):
        ent = entries_of(ring)
        ok, why = sc.ring_simple_exact(ent)
        order, st, why2 = list(range(len(ent))), 0, why
        if not ok:
            order = resort_order(ent)
            ok2, why2 = sc.ring_simple_exact(ent[order])
            st = 1 if ok2 else 2
        idx += [int(off[p]) + k for k in order]
        status.append(st)
        before.append(why)
        after.append(why2)
    idx = np.array(idx, np.int64)
    status = np.array(status, np.int8)
    return {"ring_offsets": off, "xy": xy[idx].reshape(-1, 2), "vertex_index": idx, "status": status,
            "reason_before": np.array(before, np.int32).reshape(-1, 3), "reason_after": np.array(after, np.int32).reshape(-1, 3),
            "counters": np.array([(status > 0).sum(), (status == 1).sum(), (status == 2).sum()], np.int64)}


# ---------------------------------------------------------------- cases: sizes ---
def shuffled(ring, seed):
    ent = entries_of(ring)
    return ent[np.random.default_rng(seed).permutation(len(ent))]


def sized_rings():
    """a shuffled ragged star at every size of SIZES; every other one with coordinates off the grid, so that the centre and
    the differences round"""
    out = []
    for k, n in enumerate(SIZES):
        ring = sc.star_ring(n, 300 + n)
        if k % 2:
            ring = ring * 0.3183098861837907 + np.array([1234.567, -89.0123])
        out.append(shuffled(ring, 400 + n))
    return out


def convex_ring(n, seed):
    """n grid vertices on a circle: strictly convex, so the vertices sorted around ANY interior point are the polygon"""
    return sc.star_ring(n, seed, r_lo=1.0, r_hi=1.0, scale=1.5e7)


# ---------------------------------------------------------------- cases: hand-worked and adversarial ---
def balanced(vectors, tail=()):
    """(1, 0), (-2, 0), then v, -v for every vector, then ``tail`` (zero vectors): the centre is exactly (0, 0) -- vertex 0
    counts twice and (-2, 0) takes that back, v and -v sit in neighbouring lanes and cancel in the first butterfly round
    -- so every difference IS its vertex and the case decides what the comparator sees."""
    ring = [(1.0, 0.0), (-2.0, 0.0)]
    for v in vectors:
        ring += [(float(v[0]), float(v[1])), (-float(v[0]), -float(v[1]))]
    ring = np.array(ring + [tuple(map(float, t)) for t in tail], np.float64)
    assert (centre(ring) == 0.0).all() and np.array_equal(differences(ring), ring)
    return ring


BOW_TIE = [(0, 0), (2, 2), (2, 0), (0, 2)]
COLLINEAR = [(0, 0), (1, 0), (2, 0), (3, 0)]
SPECIAL = {
    "centre_and_three_at_one_angle": balanced([(2, 2), (1, 1), (3, 3)], tail=[(0, 0)]),
    "negative_x_ray": balanced([(5, 0), (3, 1)]),
    "two_at_one_angle": balanced([(2, 4), (1, 2)]),
    "duplicates": balanced([(1, 1), (1, 1)]),
    "collinear": np.array(COLLINEAR, np.float64),
    "bow_tie": np.array(BOW_TIE, np.float64),
    "bow_tie_closed": np.array(BOW_TIE + BOW_TIE[:1], np.float64),
    "closed_with_a_twin_inside": np.array([(0, 0), (4, 0), (0, 0), (4, 4), (0, 4), (0, 0)], np.float64),
}
SPECIAL_ORDER = {                                                    # worked by hand
    "centre_and_three_at_one_angle": [5, 3, 7, 8, 0, 4, 2, 6, 1],    # (-1,-1) (-2,-2) (-3,-3) | (0,0) (1,0) | (1,1) (2,2) (3,3) | (-2,0)
    "negative_x_ray": [5, 0, 2, 4, 1, 3],                            # (-3,-1) | (1,0) (5,0) | (3,1) | (-2,0) (-5,0)
    "two_at_one_angle": [5, 3, 0, 4, 2, 1],                          # (-1,-2) (-2,-4) | (1,0) | (1,2) (2,4) | (-2,0)
    "duplicates": [3, 5, 0, 2, 4, 1],                                # equal vertices by index
    "collinear": [2, 3, 1, 0],                                       # centre 1.2: 0.8, 1.8 at angle 0, then -0.2, -1.2 at pi
    "bow_tie": [0, 2, 1, 3],                                         # centre (0.8, 0.8): the square, counter-clockwise
    "bow_tie_closed": [0, 4, 2, 1, 3],                               # the closing duplicate next to its twin
    "closed_with_a_twin_inside": [0, 2, 5, 1, 3, 4],                 # centre (4/3, 4/3): vertex 0, its twin, the duplicate
}


def _exact_cross_sign(a, b):
    c = Fraction(float(a[0])) * Fraction(float(b[1])) - Fraction(float(a[1])) * Fraction(float(b[0]))
    return (c > 0) - (c < 0)


def naive_failures(kind, count=6):
    """``count`` pairs (a, b) of nearly collinear vectors in the upper half-plane, a at the lower ring index, that the naive
    comparator ``kind`` orders wrongly: ``"cross"``, the sign of the float64 ``a.x * b.y - a.y * b.x``; ``"atan2"``, the
    float64 ``arctan2`` key with ties by index.  Asserted here: the exact order differs from the naive one."""
    rng = np.random.default_rng(5 if kind == "cross" else 6)
    out = []
    for _ in range(100000):
        a = rng.random(2) + 1.0
        b = a * (rng.random() + 1.0)                                 # a scaled and rounded: a hair off a's direction
        exact = _exact_cross_sign(a, b)
        if exact == 0:
            continue
        a_first = exact > 0
        if kind == "cross":
            naive = float(a[0] * b[1] - a[1] * b[0])
            naive_first = naive > 0.0 if naive != 0.0 else True      # a tie: by index
        else:
            ka, kb = np.arctan2(a[1], a[0]), np.arctan2(b[1], b[0])
            naive_first = bool(ka <= kb)
        if naive_first != a_first:
            out.append((a, b))
            if len(out) == count:
                break
    assert len(out) == count, (kind, len(out))
    return out


def naive_failure_rings(kind, count=6):
    """one balanced ring per pair: a at index 2, b at index 4, their negatives in the lower half-plane"""
    rings = []
    for a, b in naive_failures(kind, count):
        ring = balanced([a, b])
        order = resort_order(ring)
        assert (order.index(2) < order.index(4)) == (_exact_cross_sign(a, b) > 0)
        rings.append(ring)
    return rings


# ---------------------------------------------------------------- cases: numpy's own order ---
def separated_grid_ring(n, seed, min_gap=1e-9):
    """n integer vertices below 2^20 whose angles around numpy's centre differ pairwise by more than ``min_gap`` and none of
    which is the centre; asserts that the contract's centre has the bits of ``coords.mean(axis=0)`` of the closed ring"""
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        ring = rng.integers(0, 1 << 20, (n, 2)).astype(np.float64)
        closed = np.vstack([ring, ring[:1]])
        c = closed.mean(axis=0)
        ang = np.sort(np.arctan2(ring[:, 1] - c[1], ring[:, 0] - c[0]))
        gaps = np.diff(np.concatenate([ang, ang[:1] + 2.0 * np.pi]))
        if gaps.min() > min_gap and not (ring == c).all(axis=1).any():
            assert (np.abs(ring) < (1 << 20)).all() and centre(ring).tobytes() == c.tobytes()
            return ring
    raise AssertionError("no ring with separated angles found")


def numpy_order(ring):
    """the reference's resort_coordinates: argsort of arctan2 around the mean of the CLOSED sequence; the duplicate dropped"""
    ring = entries_of(ring)
    closed = np.vstack([ring, ring[:1]])
    c = closed.mean(axis=0)
    order = np.argsort(np.arctan2(closed[:, 1] - c[1], closed[:, 0] - c[0]))
    return [int(k) for k in order if k != len(ring)]
