"""The CPU oracle and the scenes of the nearest-boundaries tests (plain numpy: no product import).

For every (point, polygon) the oracle asks ``polygon_join_cases.match_f64`` -- float64 on coordinates translated to the
ring's first vertex, the operations of the device code in their order -- for the predicate's answer, ``dist2`` and
``parity``.  The CANDIDATES of a point are the polygons the predicate pairs it with (tests/test_nearest_cases.py pins the
set to ``join_f64`` and, on the named cases, to the exact rational ``join_exact``), each with the key

    s = 0 if dist2 == 0 else (-dist2 if parity else dist2)

and the result keeps, per point, the k smallest by (s, polygon id): deeper inside first, then nearer outside, ties to the
lower id.
"""
import functools

import numpy as np

import morphology_cases as mc
import polygon_join_cases as pc

COUNTER_NAMES = ("n_pairs", "n_kept", "n_truncated_points", "max_count")
ORIGIN = pc.ORIGIN
PRED_COLUMN = {"contains": 0, "intersects": 1}


# ---------------------------------------------------------------- the oracle ---
def candidates(points, rings, dists, predicate: str) -> dict:
    """every candidate pair -> {"point", "polygon" int64 [E], "dist2" float64 [E], "parity" bool [E], "s" float64 [E]},
    sorted by (point, s, polygon): a point's candidates in rank order"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    dists = np.broadcast_to(np.asarray(dists, dtype=np.float64), (len(rings),))
    cols = {"point": [], "polygon": [], "dist2": [], "parity": []}
    for p, ring in enumerate(rings):
        if len(points) == 0:
            break
        res = pc.match_f64(points, ring, float(dists[p]))
        idx = np.flatnonzero(res[PRED_COLUMN[predicate]])
        cols["point"].append(idx)
        cols["polygon"].append(np.full(len(idx), p, dtype=np.int64))
        cols["dist2"].append(res[2][idx])
        cols["parity"].append(res[3][idx])
    out = {"point": np.concatenate(cols["point"] + [np.zeros(0, dtype=np.int64)]).astype(np.int64),
           "polygon": np.concatenate(cols["polygon"] + [np.zeros(0, dtype=np.int64)]).astype(np.int64),
           "dist2": np.concatenate(cols["dist2"] + [np.zeros(0)]).astype(np.float64),
           "parity": np.concatenate(cols["parity"] + [np.zeros(0, dtype=bool)]).astype(bool)}
    out["s"] = np.where(out["dist2"] == 0.0, 0.0, np.where(out["parity"], -out["dist2"], out["dist2"]))
    order = np.lexsort((out["polygon"], out["s"], out["point"]))    # by value: -0.0 and +0.0 tie (s is +0.0 anyway)
    return {name: a[order] for name, a in out.items()}


def nearest(points, rings, k: int, dists=0.0, predicate: str = "intersects") -> dict:
    """the oracle of segger_amd.nearest.nearest_boundaries: numpy arrays under the product's names, ``counters`` in
    COUNTER_NAMES order"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    N, P = len(points), len(rings)
    c = candidates(points, rings, dists, predicate)
    count = np.bincount(c["point"], minlength=N).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    rank = np.arange(len(c["point"])) - start[c["point"]]            # position among the point's candidates
    keep = rank < k
    polygon = np.full((N, k), P, dtype=np.int32)
    dist2 = np.full((N, k), np.inf)
    inside = np.zeros((N, k), dtype=bool)
    polygon[c["point"][keep], rank[keep]] = c["polygon"][keep]
    dist2[c["point"][keep], rank[keep]] = c["dist2"][keep]
    inside[c["point"][keep], rank[keep]] = c["parity"][keep]
    counters = np.array([len(c["point"]), int(np.minimum(count, k).sum()), int((count > k).sum()), int(count.max()) if N else 0],
                        dtype=np.int64)
    return {"polygon": polygon, "dist2": dist2, "inside": inside, "count": count, "counters": counters}


def kept_pairs(result: dict, n_polygons: int) -> np.ndarray:
    """the kept (point, polygon) of a result as int64 [E, 2] sorted by (point, polygon)"""
    polygon = np.asarray(result["polygon"]).astype(np.int64)
    row = np.broadcast_to(np.arange(polygon.shape[0])[:, None], polygon.shape)
    keep = polygon != n_polygons
    a = np.stack([row[keep], polygon[keep]], axis=1).reshape(-1, 2)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def signed_distance(result: dict) -> np.ndarray:
    return np.where(result["inside"], -1.0, 1.0) * np.sqrt(result["dist2"])


def erosion_mask(result: dict, d: float) -> np.ndarray:
    """[N, k] bool: the point lies in the kept polygon shrunk by d (closed)"""
    return result["inside"] & (result["dist2"] >= np.float64(d) * np.float64(d))


def min_key_gap(points, rings, dists, predicate: str) -> float:
    """the smallest difference between the keys of two candidates of one point (inf without such a pair): above zero, the
    rank of every candidate is decided without the polygon id"""
    c = candidates(points, rings, dists, predicate)
    same = c["point"][1:] == c["point"][:-1]
    gaps = (c["s"][1:] - c["s"][:-1])[same]
    return float(gaps.min()) if len(gaps) else float("inf")


# ---------------------------------------------------------------- the hand-worked cases ---
def square(x0, y0, side) -> np.ndarray:
    return np.array([[x0, y0], [x0 + side, y0], [x0 + side, y0 + side], [x0, y0 + side]], dtype=np.float64) + ORIGIN


def at(*xy) -> np.ndarray:
    return np.asarray(xy, dtype=np.float64).reshape(-1, 2) + ORIGIN


def hand_unit_square() -> tuple:
    """one unit square; a point inside, one outside at distance 1/2, one on the right edge, one on the left edge
    -> (rings, points).  By hand: dist2 = 1/16, 1/4, 0, 0; parity = True, False, False (the crossing must lie STRICTLY to
    the right), True (the right edge is crossed)"""
    return (square(0.0, 0.0, 1.0),), at([0.5, 0.25], [1.5, 0.5], [1.0, 0.5], [0.0, 0.5])


def hand_nested() -> tuple:
    """[0, 4]^2 (id 0) around [1, 3]^2 (id 1) and the point (2, 2), inside both: dist2 = 4 and 1, s = -4 and -1, so the
    outer ring, in which the point is deeper, ranks first; the point (0.5, 2) is inside the outer ring only (s = -1/4) and
    1/2 left of the inner one (s = +1/4)"""
    return (square(0.0, 0.0, 4.0), square(1.0, 1.0, 2.0)), at([2.0, 2.0], [0.5, 2.0])


def hand_twins() -> tuple:
    """three rings, 0 and 2 the same unit square, 1 a larger one around them; (0.5, 0.5): the twins tie at s = -1/4 and
    rank by id, the larger square (s = -9/4) comes first"""
    return (square(0.0, 0.0, 1.0), square(-1.0, -1.0, 3.0), square(0.0, 0.0, 1.0)), at([0.5, 0.5])


def hand_shared_vertex() -> tuple:
    """[0, 1]^2 (id 0) and [1, 2]^2 (id 1) meet in the vertex (1, 1), where the point is: s = 0 twice, ranked by id.  The
    parity differs: no edge of id 0 crosses strictly to the right of the point; of id 1 the right edge does, the point being
    level with its lower end (the half-open rule counts a.y <= t.y < b.y)"""
    return (square(0.0, 0.0, 1.0), square(1.0, 1.0, 1.0)), at([1.0, 1.0])


# ---------------------------------------------------------------- the scenes ---
STACK_COPIES = 40
STACK_STEP = 1.0 / 64


@functools.lru_cache(maxsize=None)
def scene_stack(k: int, lane_max: int = 32) -> tuple:
    """STACK_COPIES unit squares, copy m shifted by m / 64 in x; the point j at x = (j + 1/2) / 64, y = 1/2 lies in the
    copies 0 .. j and in no other, so its count is j + 1 (buffer 0): counts 1, k - 1, k, k + 1, lane_max, lane_max + 1 and
    STACK_COPIES, and one point far away with count 0 -> (rings, points, counts).  A point's distances to the left and
    the right side of a copy add up to 1, so the copies rank by how close to 1/2 they are, and two copies mirror each other
    at the top of the last point's list: a tie that the lower id wins"""
    rings = tuple(square(m * STACK_STEP, 0.0, 1.0) for m in range(STACK_COPIES))
    js = sorted({0, max(k - 2, 0), k - 1, k, lane_max - 1, lane_max, STACK_COPIES - 1})
    points = at(*[[(j + 0.5) * STACK_STEP, 0.5] for j in js], [500.0, 500.0])
    return rings, points, np.array([j + 1 for j in js] + [0])


def field_dists(rings, ratio: float) -> np.ndarray:
    """sqrt(area / pi) * ratio of every ring (float64; the shoelace sum of these coordinates is exact), as
    prediction_graph_shape grows them"""
    area = np.array([mc.props_f64(r)["area"] for r in rings])
    return np.where(np.isnan(area), 0.0, np.sqrt(area / np.pi) * ratio)
