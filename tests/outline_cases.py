"""The oracle and the case list of the concave outline tests (numpy and scipy: no product import).

``outline(points, connectivity)`` restates the reference's ``_CellOutline(points).refine(connectivity).polygon()``
(``src/segger/export/boundary.py:57-154``) on ``scipy.spatial.Delaunay``'s simplices: angles and lengths with the
reference's numpy formulas, ``d_max`` by ``cKDTree``, the reference's SEQUENTIAL ``_prune`` (``prune_sequential``), and --
the one part that is restated from knowledge of shapely and not verified against it -- ``polygonize`` as "one polygon per
edge-connected piece of the surviving triangles, dangling edges ignored", of which the largest is kept.  The ring comes back
open, counter-clockwise from its lexicographically lowest vertex, every rim vertex included.

``prune_parallel`` is the form the device runs: rounds that remove every triangle with a rim edge satisfying the (static)
predicate, to the fixed point.  ``check_case`` asserts that both leave the same triangles, and the conditions under which
the device must reproduce the ring bit for bit:

* coordinates are multiples of 1/16, span fewer than 2^11 such steps per cell and are below 2^20: every orient2d and
  incircle of the device is then exact in float64;
* in integers: every scipy triangle has positive area and a STRICTLY empty circumcircle (the triangulation is unique), and
  the component areas are pairwise distinct (the tie rule, which the reference leaves to GEOS, is never used);
* no edge length is within 1e-9 (relative) of a length threshold and no angle within 1e-9 degrees of 90 or ``max_angle``
  (an ulp of difference between numpy's and the device's sqrt / acos cannot flip a predicate) -- EXCEPT an exact tie: a
  length whose double equals the threshold's, and an angle whose integer dot product is exactly 0.  With
  ``connectivity = 0.5`` the first threshold IS ``d_max``, the length of some edge, so that tie is in every cell; and a
  grid holds exact right angles, which no seed avoids among the 4000 triangles of a MAX_POINTS cell.  Both ties are decided
  without rounding on either side: the same correctly rounded sqrt of the same exact sum, and ``acos(0.0) * (180 / pi)``,
  which is 90.0 (asserted for numpy here; the device's ring would differ otherwise).  Nothing within 1e-9 that is not such
  a tie is accepted.
"""
import functools

import numpy as np
from scipy.spatial import Delaunay, cKDTree

MAX_POINTS = 2048                   # SEGGER_OUTLINE_MAX_POINTS
GRID = 16                           # coordinates are multiples of 1 / GRID
CONNECTIVITIES = (0.5, 1.0, 2.0)


# ---------------------------------------------------------------- the reference's rule, restated ---
def _as_float64(points) -> np.ndarray:
    return np.asarray(points, dtype=np.float64).reshape(-1, 2) + 0.0          # -0.0 -> +0.0, as the device reads it


def triangle_angles(points, simplices):
    p0, p1, p2 = points[simplices[:, 0]], points[simplices[:, 1]], points[simplices[:, 2]]

    def angle(u, v):
        cos = (u * v).sum(1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1) + 1e-12)
        return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))

    return np.stack([angle(p1 - p0, p2 - p0), angle(p0 - p1, p2 - p1), angle(p0 - p2, p1 - p2)], 1)


def simplex_edges(simplex):
    return [tuple(sorted((int(simplex[i]), int(simplex[(i + 1) % 3])))) for i in range(3)]


class State:
    """what ``_CellOutline.__init__`` builds, on the distinct points (qhull leaves a duplicate out of its simplices; the
    duplicates only enter d_max, where they make a nearest-neighbour distance 0)"""

    def __init__(self, points):
        p = _as_float64(points)
        self.all_points = p
        self.points = np.unique(p, axis=0)                                   # sorted by (x, y): the device's vertex order
        self.simplices = None
        if len(self.points) < 3:
            return
        q = np.round(self.points * GRID).astype(np.int64)
        if _collinear(q):                                                    # qhull raises, the reference returns None
            return
        s = Delaunay(self.points).simplices.astype(np.int64)
        a, b, c = q[s[:, 0]], q[s[:, 1]], q[s[:, 2]]
        flip = ((b - a)[:, 0] * (c - a)[:, 1] - (b - a)[:, 1] * (c - a)[:, 0]) < 0
        s[flip] = s[flip][:, [0, 2, 1]]                                      # counter-clockwise
        self.simplices = s
        dist, _ = cKDTree(p).query(p, k=2)
        self.d_max = float(dist[:, 1].max())
        self.angles = triangle_angles(self.points, s)
        self.edges = {}
        for ti, simplex in enumerate(s):
            for k, edge in enumerate(simplex_edges(simplex)):
                if edge not in self.edges:
                    u, v = edge
                    self.edges[edge] = {"tri": {}, "length": float(np.linalg.norm(self.points[u] - self.points[v]))}
                self.edges[edge]["tri"][ti] = float(self.angles[ti][(k + 2) % 3])


def _collinear(q) -> bool:
    d = q - q[0]
    k = int(np.argmax((d * d).sum(1)))
    return not (d[:, 0] * d[k, 1] - d[:, 1] * d[k, 0]).any()


def predicates(st: State, connectivity: float):
    d_max = st.d_max
    max_angle = 180 - (180 / 16) / connectivity
    return (lambda length, angle: length > 2 * connectivity * d_max,
            lambda length, angle: (length > 1.5 * connectivity * d_max and angle > 90) or angle > max_angle)


def prune_sequential(st: State, connectivity: float):
    """the reference's refine(): -> (surviving triangle ids, rim edges len(tri) < 2 as sorted index pairs)"""
    edges = {e: {"tri": dict(i["tri"]), "length": i["length"]} for e, i in st.edges.items()}
    degree = np.bincount(np.array(list(edges), dtype=np.int64).ravel(), minlength=len(st.points))

    def drop(edge):
        a, b = edge
        if degree[a] <= 1 or degree[b] <= 1:
            return False
        del edges[edge]
        degree[a] -= 1
        degree[b] -= 1
        return True

    for pred in predicates(st, connectivity):
        boundary = [e for e in edges if len(edges[e]["tri"]) < 2]
        changed = True
        while changed:
            changed, nxt = False, []
            for edge in boundary:
                info = edges.get(edge)
                if info is None:
                    continue
                if not info["tri"]:
                    if not drop(edge):
                        nxt.append(edge)
                    continue
                ti = next(iter(info["tri"]))
                if pred(info["length"], info["tri"][ti]) and drop(edge):
                    for other in simplex_edges(st.simplices[ti]):
                        if other != edge and other in edges:
                            edges[other]["tri"].pop(ti, None)
                            nxt.append(other)
                    changed = True
                else:
                    nxt.append(edge)
            boundary = nxt
    alive = sorted({ti for i in edges.values() for ti in i["tri"]})
    rim = sorted(e for e, i in edges.items() if len(i["tri"]) < 2)
    return alive, rim


def prune_parallel(st: State, connectivity: float):
    """rounds of "remove every triangle with a rim edge satisfying the predicate", to the fixed point, phase by phase"""
    alive = np.ones(len(st.simplices), dtype=bool)
    for pred in predicates(st, connectivity):
        flag = {(e, ti): pred(i["length"], ang) for e, i in st.edges.items() for ti, ang in i["tri"].items()}
        while True:
            gone = [ti for e, i in st.edges.items() for ti in i["tri"]
                    if alive[ti] and flag[(e, ti)] and sum(alive[t] for t in i["tri"]) == 1]
            if not gone:
                break
            alive[gone] = False
    return sorted(np.flatnonzero(alive).tolist())


def components(st: State, alive):
    """edge-connected pieces of the alive triangles -> list of (twice the area in grid units, triangle ids)"""
    parent = {t: t for t in alive}

    def find(t):
        while parent[t] != t:
            parent[t] = parent[parent[t]]
            t = parent[t]
        return t

    live = set(alive)
    for i in st.edges.values():
        ts = [t for t in i["tri"] if t in live]
        if len(ts) == 2:
            parent[find(ts[0])] = find(ts[1])
    q = np.round(st.points * GRID).astype(np.int64)
    groups = {}
    for t in alive:
        groups.setdefault(find(t), []).append(t)
    out = []
    for ts in groups.values():
        a, b, c = (q[st.simplices[ts][:, k]] for k in range(3))
        area2 = int((((b - a)[:, 0] * (c - a)[:, 1]) - ((b - a)[:, 1] * (c - a)[:, 0])).sum())
        out.append((area2, ts))
    return out


def ring_of(st: State, tris):
    """the rim of an edge-connected set of counter-clockwise triangles, as vertex indices, interior on the left, from the
    lowest vertex; asserts that it is one simple ring"""
    directed = {}
    for t in tris:
        s = st.simplices[t]
        for k in range(3):
            directed[(int(s[k]), int(s[(k + 1) % 3]))] = t
    rim = {a: b for (a, b) in directed if (b, a) not in directed}
    assert len(rim) == sum(1 for (a, b) in directed if (b, a) not in directed), "a pinched ring"
    start = min(rim)
    ring, v = [start], rim[start]
    while v != start:
        ring.append(v)
        v = rim[v]
        assert len(ring) <= len(rim)
    assert len(ring) == len(rim), "more than one ring"
    return ring


@functools.lru_cache(maxsize=None)
def _outline_cached(key, connectivity):
    points = np.frombuffer(key, dtype=np.float64).reshape(-1, 2)
    st = State(points)
    if st.simplices is None:
        return None
    alive, _ = prune_sequential(st, connectivity)
    if not alive:
        return None
    area2, tris = max(components(st, alive), key=lambda c: c[0])
    ring = st.points[ring_of(st, tris)]
    ring.setflags(write=False)
    return ring, area2 / (2.0 * GRID * GRID)


def outline(points, connectivity: float = 2.0):
    """-> float64 [h, 2] ring, or None when the cell has no polygon"""
    got = _outline_cached(_as_float64(points).tobytes(), float(connectivity))
    return None if got is None else got[0]


def outline_area(points, connectivity: float = 2.0) -> float:
    return _outline_cached(_as_float64(points).tobytes(), float(connectivity))[1]


# ---------------------------------------------------------------- the conditions of exactness ---
def check_case(points, connectivity: float) -> dict:
    """asserts the module docstring's conditions and the order-independence of the peel; -> a few figures"""
    p = _as_float64(points)
    q = p * GRID
    assert np.array_equal(q, np.round(q)) and np.abs(p).max() < (1 << 20), "off the grid"
    assert (q.max(0) - q.min(0)).max() < (1 << 11), "the cell spans 2^11 grid steps or more"
    st = State(p)
    if st.simplices is None:
        return {"triangles": 0}
    q = np.round(st.points * GRID).astype(np.int64)
    s = st.simplices
    a, b, c = q[s[:, 0]], q[s[:, 1]], q[s[:, 2]]
    assert ((((b - a)[:, 0] * (c - a)[:, 1]) - ((b - a)[:, 1] * (c - a)[:, 0])) > 0).all(), "a flat triangle"
    for lo in range(0, len(s), 256):                                         # incircle of every point, int64: below 2^48
        A, B, C = (x[lo:lo + 256, None, :] - q[None, :, :] for x in (a, b, c))
        det = ((A * A).sum(-1) * (B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0])
               + (B * B).sum(-1) * (C[..., 0] * A[..., 1] - C[..., 1] * A[..., 0])
               + (C * C).sum(-1) * (A[..., 0] * B[..., 1] - A[..., 1] * B[..., 0]))
        det[np.arange(len(det))[:, None], s[lo:lo + 256]] = -1                # its own corners lie on the circle
        assert (det < 0).all(), "co-circular points: the triangulation is not unique"
    max_angle = 180 - (180 / 16) / connectivity
    lengths = np.array([i["length"] for i in st.edges.values()])
    for thr in (2 * connectivity * st.d_max, 1.5 * connectivity * st.d_max):
        assert ((np.abs(lengths - thr) > 1e-9 * thr) | (lengths == thr)).all(), "a length near a threshold"
    dots = np.stack([((b - a) * (c - a)).sum(1), ((a - b) * (c - b)).sum(1), ((a - c) * (b - c)).sum(1)], 1)
    assert ((np.abs(st.angles - 90) > 1e-9) | (dots == 0)).all(), "an angle near 90"
    assert (st.angles[dots == 0] == 90.0).all(), "numpy's angle of an exact right angle is not 90.0"
    assert (np.abs(st.angles - max_angle) > 1e-9).all(), "an angle near max_angle"
    alive, _ = prune_sequential(st, connectivity)
    assert alive == prune_parallel(st, connectivity), "the order of the peel decided the result"
    comps = components(st, alive)
    areas = [c[0] for c in comps]
    assert len(set(areas)) == len(areas), "components of equal area"
    return {"triangles": len(s), "alive": len(alive), "components": len(comps)}


def hull_area(points) -> float:
    import boundaries_cases as bc
    h = bc.hull(_as_float64(points) * GRID)
    return bc.area2_exact(h) / (2.0 * GRID * GRID)


# ---------------------------------------------------------------- the cells ---
def cloud(n: int, seed: int, half: int = 600, centre=(0.0, 0.0)) -> np.ndarray:
    """n DISTINCT points on the 1/16 grid, uniform in a square of 2 half + 1 grid steps"""
    rng = np.random.default_rng(seed)
    got = np.zeros((0, 2), dtype=np.int64)
    while len(got) < n:
        got = np.unique(np.concatenate([got, rng.integers(-half, half + 1, (2 * n, 2))]), axis=0)
    return rng.permutation(got)[:n].astype(np.float64) / GRID + np.asarray(centre, dtype=np.float64)


def crescent(n: int = 150, seed: int = 3) -> np.ndarray:
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0.15 * np.pi, 1.85 * np.pi, 4 * n)
    r = rng.uniform(35.0, 55.0, 4 * n)
    pts = np.unique(np.round(np.stack([r * np.cos(ang), r * np.sin(ang)], 1) * GRID), axis=0)
    return rng.permutation(pts)[:n] / GRID


def two_blobs(gap: float, seed: int, n: int = 40, bridge=()) -> np.ndarray:
    """two blobs of n points, `gap` apart, and the points of `bridge` between them"""
    rng = np.random.default_rng(seed)
    left = np.round(rng.uniform(-10.0, 10.0, (n, 2)) * GRID) / GRID + [-10.0 - gap / 2, 0.0]
    right = np.round(rng.uniform(-8.0, 8.0, (n - 8, 2)) * GRID) / GRID + [8.0 + gap / 2, 0.0]
    pts = np.concatenate([left, right, np.asarray(bridge, dtype=np.float64).reshape(-1, 2)])
    return np.unique(pts, axis=0)


@functools.lru_cache(maxsize=None)
def cells() -> dict:
    """cell id -> points, the cells every test shares; ids 0, 3 and 30 .. 39 own no row"""
    dup = cloud(40, 21, 200, (50.0, -20.0))
    return {
        1: np.array([[0.0, 0.0], [4.0, 0.0], [1.0, 3.0]]),                                  # 3 points, kept
        2: np.array([[0.0, 0.0], [10.0, 0.0], [5.0, 0.125]]),                               # 3 points, thin: all pruned
        4: np.array([[0.0, 0.0], [4.0, 0.0], [5.0, 3.0], [1.0, 2.0]]),                      # 4 points, not co-circular
        5: np.array([[3.0, 4.0], [3.0, 4.0], [-0.0, 1.0], [0.0, 1.0]]),                     # 2 distinct points
        6: np.array([[0.0, 0.0], [1.5, 1.5], [3.0, 3.0], [-2.0, -2.0]]),                    # collinear
        7: np.array([[7.0, -2.0]] * 5),                                                     # one point, five times
        8: np.concatenate([dup, dup[:7], dup[:3], dup[20:25]]),                             # duplicates, rim and interior
        9: crescent(),
        10: two_blobs(6.0, 5, bridge=[[0.0, 0.5]]),                                         # the neck is severed
        11: two_blobs(14.0, 6),                                                             # two pieces apart
        12: two_blobs(0.0, 9, bridge=[[0.0, 0.0]]),
        13: cloud(63, 63, 300, (-100.0, 100.0)),
        14: cloud(64, 64, 300, (0.0, 100.0)),
        15: cloud(65, 65, 300, (100.0, 100.0)),
        16: cloud(255, 255, 500, (0.0, -200.0)),                                            # the two sides of the route threshold
        17: cloud(256, 256, 500, (100.0, -200.0)),
        18: cloud(257, 257, 500, (200.0, -200.0)),
    }


@functools.lru_cache(maxsize=None)
def big_cells() -> dict:
    """MAX_POINTS - 1 and MAX_POINTS distinct points, thinly spread (1000 x 1000 grid steps hold them)"""
    return {0: cloud(MAX_POINTS - 1, 2047, 1000), 1: cloud(MAX_POINTS, 2049, 1000, (300.0, 0.0))}


def too_big_cell() -> np.ndarray:
    return cloud(MAX_POINTS + 1, 2049, 1000)


N_CELLS = 60


@functools.lru_cache(maxsize=None)
def scene_cells() -> dict:
    """about 40 cells: the shared ones and random clouds of 3 .. 120 points"""
    out = dict(cells())
    rng = np.random.default_rng(40)
    for k, n in enumerate(rng.integers(3, 121, 23)):
        out[20 + k + (k > 9) * 10] = cloud(int(n), 500 + k, 250, (40.0 * k - 400.0, 300.0))
    return out


@functools.lru_cache(maxsize=None)
def scene(seed: int = 0):
    """(xy, cell int32, keep) of scene_cells, shuffled; rows with negative ids, rows masked out (some in a cell's id)"""
    rng = np.random.default_rng(seed)
    cs = scene_cells()
    noise = cloud(300, 77, 900)
    xy = np.concatenate(list(cs.values()) + [noise])
    ids = np.concatenate([np.full(len(p), c) for c, p in cs.items()] + [np.where(np.arange(300) % 3 == 0, 14, np.where(np.arange(300) % 3 == 1, -1, -7))])
    keep = np.concatenate([np.ones(len(xy) - 300, dtype=bool), np.arange(300) % 3 != 0])    # the noise rows of cell 14 are masked
    perm = rng.permutation(len(xy))
    return np.ascontiguousarray(xy[perm]), ids[perm].astype(np.int32), keep[perm]


def expected(cs: dict, connectivity: float = 2.0, smoothing: int = 0):
    """(ring_offsets, xy, cell_ids, n_transcripts, n_dropped) the device must return for these cells"""
    import boundaries_cases as bc
    rings = {c: outline(p, connectivity) for c, p in cs.items()}
    kept = [c for c in sorted(cs) if rings[c] is not None]
    out = [bc.chaikin(rings[c], smoothing) for c in kept]
    offsets = np.zeros(len(kept) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in out])
    return (offsets, np.concatenate(out + [np.zeros((0, 2))]), np.array(kept, dtype=np.int32),
            np.array([len(cs[c]) for c in kept], dtype=np.int64), len(cs) - len(kept))
