"""The canonical oracle and the cells of the large-cell outline tests (numpy and scipy: no product import).

A cell of several thousand points on the 1/16 grid inside fewer than 2^11 grid steps holds co-circular quadruples, so its
Delaunay triangulation is not unique and ``outline_cases.check_case`` refuses it.  ``canonical_state`` removes the choice the
way the device documents it: scipy's triangles that share an edge and whose opposite vertex has an exactly zero integer
``incircle`` are merged into their co-circular polygons, and every polygon is re-triangulated as the fan from its lowest
(x, then y) vertex.  On that triangulation run ``outline_cases``' own angles, ``prune_sequential`` / ``prune_parallel``,
``components`` and ``ring_of``.  ``check_large`` asserts ``check_case``'s other conditions in the same way: the grid, the span
below 2^11 steps, no flat triangle, no length or angle within 1e-9 of a threshold unless an exact tie, the sequential peel
equal to the parallel one, distinct component areas.  (That no point lies strictly inside a circumcircle is scipy's word
here; ``check_case`` tests it for the cells it accepts, at a cost quadratic in the points.)

Seeds.  Every cell below passed ``check_large`` with the first seed tried at connectivity 2.0, the one the tests use:
``limit_cell`` is ``outline_cases.too_big_cell()`` (seed 2049; it also passes ``check_case`` at all three connectivities),
``edge_ids_cell`` seed 11500, ``vertex_ids_cell`` seed 65537, ``repeated_cell`` seed 4.
"""
import functools

import numpy as np

import outline_cases as oc

GOLDEN_CASES = ("edge_ids", "vertex_ids")


def _incircle_int(q, a, b, c, d):
    A, B, C = q[a] - q[d], q[b] - q[d], q[c] - q[d]
    return ((A * A).sum(-1) * (B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0])
            + (B * B).sum(-1) * (C[..., 0] * A[..., 1] - C[..., 1] * A[..., 0])
            + (C * C).sum(-1) * (A[..., 0] * B[..., 1] - A[..., 1] * B[..., 0]))


def canonical_simplices(points, simplices):
    """counter-clockwise triangles over points sorted by (x, y) -> the same with every co-circular polygon as the fan from
    its lowest vertex"""
    q = np.round(points * oc.GRID).astype(np.int64)
    s = np.asarray(simplices, dtype=np.int64)
    T = len(s)
    # directed edge (a, b) of triangle t with opposite vertex c, sorted so that twins meet
    a = s[:, [0, 1, 2]].ravel()
    b = s[:, [1, 2, 0]].ravel()
    c = s[:, [2, 0, 1]].ravel()
    t = np.repeat(np.arange(T), 3)
    key = np.minimum(a, b) * (len(points) + 1) + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    i, j = order[:-1][same], order[1:][same]                                 # the two sides of every interior edge
    zero = _incircle_int(q, a[i], b[i], c[i], c[j]) == 0
    parent = np.arange(T)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(t[i][zero].tolist(), t[j][zero].tolist()):
        parent[find(x)] = find(y)
    groups = {}
    for x in sorted(set(t[i][zero].tolist()) | set(t[j][zero].tolist())):
        groups.setdefault(find(x), []).append(x)
    keep = np.ones(T, dtype=bool)
    fans = []
    for ts in groups.values():
        keep[ts] = False
        directed = {(int(s[x][k]), int(s[x][(k + 1) % 3])) for x in ts for k in range(3)}
        rim = {u: v for (u, v) in directed if (v, u) not in directed}
        m = min(rim)
        ring, v = [m], rim[m]
        while v != m:
            ring.append(v)
            v = rim[v]
        assert len(ring) == len(rim) == len(ts) + 2, "a co-circular group that is not one polygon"
        fans += [(m, ring[k], ring[k + 1]) for k in range(1, len(ring) - 1)]
    return np.concatenate([s[keep], np.array(fans, dtype=np.int64).reshape(-1, 3)])


def canonical_state(points) -> oc.State:
    st = oc.State(points)
    if st.simplices is None:
        return st
    s = canonical_simplices(st.points, st.simplices)
    st.simplices = s
    st.angles = oc.triangle_angles(st.points, s)
    st.edges = {}
    for ti, simplex in enumerate(s.tolist()):
        for k in range(3):
            u, v = simplex[k], simplex[(k + 1) % 3]
            edge = (u, v) if u < v else (v, u)
            info = st.edges.get(edge)
            if info is None:
                info = st.edges[edge] = {"tri": {}, "length": float(np.linalg.norm(st.points[u] - st.points[v]))}
            info["tri"][ti] = float(st.angles[ti][(k + 2) % 3])
    return st


def prune_parallel_fast(st: oc.State, connectivity: float):
    """``outline_cases.prune_parallel`` with the rim found per round from arrays, for cells of 10^5 triangles"""
    s = st.simplices
    T = len(s)
    edge_ids = {e: k for k, e in enumerate(st.edges)}
    side = np.full((len(edge_ids), 2), -1, dtype=np.int64)                   # the triangles of an edge
    tri_edge = np.zeros((T, 3), dtype=np.int64)
    flags = [np.zeros((T, 3), dtype=bool), np.zeros((T, 3), dtype=bool)]
    preds = oc.predicates(st, connectivity)
    for e, info in st.edges.items():
        for slot, (ti, ang) in enumerate(info["tri"].items()):
            side[edge_ids[e], slot] = ti
            k = [tuple(sorted((int(s[ti][m]), int(s[ti][(m + 1) % 3])))) for m in range(3)].index(e)
            tri_edge[ti, k] = edge_ids[e]
            for p in range(2):
                flags[p][ti, k] = preds[p](info["length"], ang)
    alive = np.ones(T, dtype=bool)
    padded = np.append(alive, False)                                         # index -1: no triangle
    for p in range(2):
        while True:
            padded[:T] = alive
            n_alive = padded[side].sum(1)                                    # per edge
            gone = alive & (flags[p] & (n_alive[tri_edge] == 1)).any(1)
            if not gone.any():
                break
            alive &= ~gone
    return np.flatnonzero(alive).tolist()


def outline_canonical(points, connectivity: float = 2.0, check: bool = False):
    """-> (ring float64 [h, 2] or None, area, triangles); with ``check`` the conditions of exactness are asserted"""
    st = canonical_state(points)
    if st.simplices is None:
        return None, 0.0, 0
    alive, _ = oc.prune_sequential(st, connectivity)
    if check:
        _check(st, alive, connectivity)
    if not alive:
        return None, 0.0, len(st.simplices)
    area2, tris = max(oc.components(st, alive), key=lambda c: c[0])
    return st.points[oc.ring_of(st, tris)], area2 / (2.0 * oc.GRID * oc.GRID), len(st.simplices)


def _check(st, alive, connectivity):
    p = st.all_points
    q = p * oc.GRID
    assert np.array_equal(q, np.round(q)) and np.abs(p).max() < (1 << 20), "off the grid"
    assert (q.max(0) - q.min(0)).max() < (1 << 11), "the cell spans 2^11 grid steps or more"
    q = np.round(st.points * oc.GRID).astype(np.int64)
    s = st.simplices
    a, b, c = q[s[:, 0]], q[s[:, 1]], q[s[:, 2]]
    assert ((((b - a)[:, 0] * (c - a)[:, 1]) - ((b - a)[:, 1] * (c - a)[:, 0])) > 0).all(), "a flat triangle"
    max_angle = 180 - (180 / 16) / connectivity
    lengths = np.array([i["length"] for i in st.edges.values()])
    for thr in (2 * connectivity * st.d_max, 1.5 * connectivity * st.d_max):
        assert ((np.abs(lengths - thr) > 1e-9 * thr) | (lengths == thr)).all(), "a length near a threshold"
    dots = np.stack([((b - a) * (c - a)).sum(1), ((a - b) * (c - b)).sum(1), ((a - c) * (b - c)).sum(1)], 1)
    assert ((np.abs(st.angles - 90) > 1e-9) | (dots == 0)).all(), "an angle near 90"
    assert (st.angles[dots == 0] == 90.0).all(), "numpy's angle of an exact right angle is not 90.0"
    assert (np.abs(st.angles - max_angle) > 1e-9).all(), "an angle near max_angle"
    assert alive == prune_parallel_fast(st, connectivity), "the order of the peel decided the result"
    areas = [c[0] for c in oc.components(st, alive)]
    assert len(set(areas)) == len(areas), "components of equal area"


def check_large(points, connectivity: float = 2.0):
    return outline_canonical(points, connectivity, check=True)


# ---------------------------------------------------------------- the cells ---
def limit_cell() -> np.ndarray:
    """MAX_POINTS + 1 distinct points"""
    return oc.too_big_cell()


@functools.lru_cache(maxsize=None)
def edge_ids_cell() -> np.ndarray:
    """11 500 distinct points: more than 21 846 triangles, directed-edge ids pass 65 535"""
    return oc.cloud(11500, 11500, 1000)


@functools.lru_cache(maxsize=None)
def vertex_ids_cell() -> np.ndarray:
    """65 537 distinct points within 2001 x 2001 grid steps: vertex ids pass 65 535"""
    return oc.cloud(65537, 65537, 1000)


def repeated_cell() -> np.ndarray:
    """the 2049 points of limit_cell shifted, each but one twice: 4097 rows.  With EVERY point repeated d_max is 0 and
    nothing survives the peel, so the loneliest point stays single: d_max is its distance, and dropping the flag of any
    other point cannot raise it -- but taking a repeated point's distance for 0 where it should not be would lower it."""
    from scipy.spatial import cKDTree
    p = limit_cell() + [500.0, 0.0]
    lonely = int(np.argmax(cKDTree(p).query(p, k=2)[0][:, 1]))
    return np.random.default_rng(4).permutation(np.concatenate([p, np.delete(p, lonely, axis=0)]))


def many_rows_few_points() -> np.ndarray:
    """2048 distinct points, 2500 rows: stays on the LDS route"""
    p = oc.big_cells()[1]
    return np.random.default_rng(5).permutation(np.concatenate([p, p[:452]]))


def expected(cs: dict, connectivity: float = 2.0, smoothing: int = 0):
    """``outline_cases.expected`` on the canonical oracle"""
    import boundaries_cases as bc
    rings = {c: outline_canonical(p, connectivity)[0] for c, p in cs.items()}
    kept = [c for c in sorted(cs) if rings[c] is not None]
    out = [bc.chaikin(rings[c], smoothing) for c in kept]
    offsets = np.zeros(len(kept) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in out])
    return (offsets, np.concatenate(out + [np.zeros((0, 2))]), np.array(kept, dtype=np.int32),
            np.array([len(cs[c]) for c in kept], dtype=np.int64), len(cs) - len(kept))
