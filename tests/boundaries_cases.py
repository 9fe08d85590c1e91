"""The oracle and the case list of the cell boundary tests (plain numpy and the standard library: no product import).

``hull(points)`` is Andrew's monotone chain with an EXACT orientation test: Python integers when every coordinate is an
integer, ``fractions.Fraction`` of the float64 values otherwise.  It returns the strict hull -- no point on an edge, one
of equal points -- counter-clockwise from the lexicographically lowest point, as coordinates, or ``None`` under the
reference's degenerate rule (``np.unique(points) < 3``, or all collinear: shapely's hull is then no Polygon).
``hull_f64`` is the same chain with float64 cross products.  ``chaikin`` is the reference's formula, iterated:
``out[2k] = 0.75 p[k] + 0.25 p[k + 1]``, ``out[2k + 1] = 0.25 p[k] + 0.75 p[k + 1]``, indices cyclic.

Every coordinate of the integer cases is below 2^20 in magnitude (``LIMIT``), where the device's float64 orientation is
exact and its ring must equal the oracle's vertex for vertex, bit for bit.
"""
import functools
from fractions import Fraction

import numpy as np

MAX_VERTS = 4096                    # SEGGER_MORPH_MAX_VERTS
CHUNK_MAX_HULL = 2048               # SEGGER_BOUNDARY_CHUNK_MAX_HULL
LIMIT = 1 << 20


# ---------------------------------------------------------------- the oracle ---
def _chain(pts, cross) -> list:
    """indices of the strict hull of pts (a list of (x, y)), counter-clockwise from the lowest (x, y)"""
    order = sorted(range(len(pts)), key=lambda i: (pts[i][0], pts[i][1]))
    uniq = [i for k, i in enumerate(order) if k == 0 or pts[i] != pts[order[k - 1]]]
    if len(uniq) <= 2:
        return uniq
    lower, upper = [], []
    for chain, seq in ((lower, uniq), (upper, uniq[::-1])):
        for i in seq:
            while len(chain) >= 2 and cross(pts[chain[-2]], pts[chain[-1]], pts[i]) <= 0:
                chain.pop()
            chain.append(i)
    return lower[:-1] + upper[:-1]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _as_float64(points) -> np.ndarray:
    return np.asarray(points, dtype=np.float64).reshape(-1, 2) + 0.0          # -0.0 -> +0.0, as the device reads it


def hull(points):
    """exact strict hull -> float64 [h, 2], or None when the cell has no polygon"""
    p = _as_float64(points)
    if np.array_equal(p, np.round(p)):
        pts = [(int(x), int(y)) for x, y in p]
    else:
        pts = [(Fraction(float(x)), Fraction(float(y))) for x, y in p]
    idx = _chain(pts, _cross)
    return p[idx] if len(idx) >= 3 else None


def hull_f64(points):
    """the same chain with float64 cross products (differences first, two products, one subtraction)"""
    p = _as_float64(points)
    idx = _chain([(float(x), float(y)) for x, y in p], _cross)
    return p[idx] if len(idx) >= 3 else None


def chaikin(ring: np.ndarray, iterations: int) -> np.ndarray:
    ring = np.asarray(ring, dtype=np.float64)
    for _ in range(iterations):
        nxt = np.roll(ring, -1, axis=0)
        out = np.empty((2 * len(ring), 2))
        out[0::2] = 0.75 * ring + 0.25 * nxt
        out[1::2] = 0.25 * ring + 0.75 * nxt
        ring = out
    return ring


def area2_exact(ring: np.ndarray) -> int:
    """twice the area of an integer ring, exactly"""
    pts = [(int(x), int(y)) for x, y in ring]
    return abs(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(pts, pts[1:] + pts[:1])))


def on_boundary(points: np.ndarray, ring: np.ndarray) -> np.ndarray:
    """which integer points lie on an edge of the integer ring (exact in int64: everything is below 2^21)"""
    p = np.asarray(points).astype(np.int64)
    a = np.asarray(ring).astype(np.int64)
    b = np.roll(a, -1, axis=0)
    e = (b - a)[None, :, :]
    w = p[:, None, :] - a[None, :, :]
    cr = e[..., 0] * w[..., 1] - e[..., 1] * w[..., 0]
    dot = w[..., 0] * e[..., 0] + w[..., 1] * e[..., 1]
    return ((cr == 0) & (dot >= 0) & (dot <= (e * e).sum(-1))).any(1)


# ---------------------------------------------------------------- the cells ---
def circle(n: int, radius: int, seed: int) -> np.ndarray:
    """n distinct integer points rounded from a circle, shuffled; radius (1 - cos(pi / n)) is far above the rounding, so
    every one of them is a strict hull vertex"""
    ang = 2 * np.pi * (np.arange(n) + 0.25) / n
    pts = np.round(radius * np.stack([np.cos(ang), np.sin(ang)], 1))
    return np.random.default_rng(seed).permutation(pts)


def cloud(n: int, seed: int, half: int = 1000, centre=(0, 0)) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.integers(-half, half + 1, (n, 2)).astype(np.float64) + np.asarray(centre, dtype=np.float64)


def chunked_cell(n: int = 9000, n_hull: int = 200, seed: int = 5) -> np.ndarray:
    """n points: n_hull on a circle and the rest inside it, shuffled so that every chunk brings hull vertices"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n - n_hull)
    r = 90000 * np.sqrt(rng.uniform(0, 1, n - n_hull))
    inner = np.round(np.stack([r * np.cos(ang), r * np.sin(ang)], 1))
    return rng.permutation(np.concatenate([circle(n_hull, 100000, seed), inner]))


def parabola(n: int = 5000) -> np.ndarray:
    """n points that are all hull vertices: the chunked route's first round ends with MAX_VERTS > CHUNK_MAX_HULL of them"""
    i = np.arange(n, dtype=np.float64) - n // 2
    return np.stack([i, i * i], 1)


@functools.lru_cache(maxsize=None)
def tiny_cells() -> dict:
    grid = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0)), -1).reshape(-1, 2)
    square = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], dtype=np.float64)
    return {
        1: np.array([[3.0, 4.0]]),                                                   # cell 0 has no row at all
        2: np.array([[0.0, 0.0], [5.0, 5.0]]),
        3: np.array([[0.0, 0.0], [2.0, 2.0], [1.0, 1.0]]),                           # collinear
        4: np.array([[7.0, -2.0]] * 5),                                              # one point, five times
        5: np.array([[0.0, 0.0], [4.0, 0.0], [1.0, 3.0]]),
        6: grid + [100.0, 100.0],                                                    # hull: its 4 corners
        7: np.concatenate([square, square, square[:2], [[5.0, 5.0], [5.0, 0.0], [-0.0, 5.0]]]) + [-300.0, 40.0],
        8: np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [3.0, 0.0], [4.0, 0.0], [2.0, 1.0]]),    # 5 collinear and one off
        9: np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [0.0, 0.0], [2.0, 2.0]]),   # collinear with duplicates
    }


ROUTE_SIZES = (63, 64, 65, MAX_VERTS - 1, MAX_VERTS, MAX_VERTS + 1)


@functools.lru_cache(maxsize=None)
def scene_cells() -> dict:
    """cell id -> points (integers as float64) of the one scene the device tests share"""
    cells = dict(tiny_cells())
    for k, n in enumerate(ROUTE_SIZES):
        cells[20 + 2 * k] = cloud(n, 100 + n, 1000, (3000 * k - 9000, 5000))
    cells[40] = chunked_cell()
    cells[41] = circle(100, 20000, 9) + [200000.0, -300000.0]                        # a hull of 100 on the LDS route
    return cells


N_CELLS = 50                        # the id domain of the scene: ids 0, 10 .. 19, 42 .. 49 and others have no row


@functools.lru_cache(maxsize=None)
def scene(seed: int = 0):
    """(xy [N, 2] float64, cell [N] int32) of scene_cells, rows interleaved at random, with unassigned rows (-1, -7)"""
    rng = np.random.default_rng(seed)
    cells = scene_cells()
    xy = np.concatenate(list(cells.values()) + [cloud(500, 77, 50000)])
    ids = np.concatenate([np.full(len(p), c) for c, p in cells.items()] + [np.where(np.arange(500) % 2, -1, -7)])
    assert np.abs(xy).max() < LIMIT
    perm = rng.permutation(len(xy))
    return np.ascontiguousarray(xy[perm]), ids[perm].astype(np.int32)


@functools.lru_cache(maxsize=None)
def scene_hulls() -> dict:
    """cell id -> exact hull, or None: computed once per process"""
    return {c: hull(p) for c, p in scene_cells().items()}


def expected(cells: dict, hulls: dict, smoothing: int = 0):
    """(ring_offsets, xy, cell_ids, n_transcripts, n_dropped) the device must return for these cells"""
    kept = [c for c in sorted(cells) if hulls[c] is not None]
    rings = [chaikin(hulls[c], smoothing) for c in kept]
    offsets = np.zeros(len(kept) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rings])
    xy = np.concatenate(rings + [np.zeros((0, 2))])
    return (offsets, xy, np.array(kept, dtype=np.int32), np.array([len(cells[c]) for c in kept], dtype=np.int64),
            len(cells) - len(kept))


@functools.lru_cache(maxsize=None)
def real_cells() -> dict:
    """seeded real coordinates on slide scale, in general position: tests/test_boundaries_oracle.py checks that the float64
    and the exact hulls of every cell are identical, so the device's must be too"""
    rng = np.random.default_rng(2024)
    return {c: rng.normal(0.0, 8.0, (n, 2)) + rng.uniform(2e4, 9e4, 2) for c, n in enumerate((3, 17, 64, 65, 300, 1500))}
