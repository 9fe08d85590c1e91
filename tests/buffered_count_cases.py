"""The CPU oracle and the scenes of the buffered-boundary count tests (plain numpy: no product import).

For every (point, polygon) the oracle asks the predicate oracles of tests/polygon_join_cases.py (``join_f64``: float64
on coordinates translated to the ring's first vertex, the operations of the device code in its order; the exact rational
``join_exact`` pins it in tests/test_buffered_count_cases.py), and builds the polygon x gene CSR with numpy:

    entry (p, g) = the number of points of gene g that match polygon p grown by dists[p]
    a point whose gene lies outside [0, n_genes) is counted in n_bad when it matches, and nowhere else

It also restates the reference's ``filter_boundaries`` (src/segger/metrics/segment.py:125-156) and the sum over regions
of ``get_buffered_counts_distributed`` in numpy.
"""
import functools

import numpy as np

import morphology_cases as mc
import polygon_join_cases as pc

COUNTER_NAMES = ("n_pairs", "nnz", "n_bad", "n_overflow_rows", "n_large_tier")
ORIGIN = pc.ORIGIN


# ---------------------------------------------------------------- the oracle ---
def pairs(points, rings, dists, predicate: str) -> np.ndarray:
    """int64 [E, 2] of (point, polygon), sorted by (point, polygon)"""
    return pc.join_f64(points, rings, np.asarray(dists, dtype=np.float64))[predicate]


def csr_from_pairs(pr: np.ndarray, gene, n_polygons: int, n_genes: int) -> dict:
    gene = np.asarray(gene).astype(np.int64)
    g = gene[pr[:, 0]]
    ok = (g >= 0) & (g < n_genes)
    key = pr[ok, 1] * n_genes + g[ok]
    uniq, cnt = np.unique(key, return_counts=True)
    row = uniq // n_genes
    indptr = np.zeros(n_polygons + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(row, minlength=n_polygons))
    return {"indptr": indptr, "indices": (uniq - row * n_genes).astype(np.int32), "counts": cnt.astype(np.int32),
            "cell_count": np.bincount(pr[ok, 1], minlength=n_polygons).astype(np.int64), "n_pairs": len(pr), "n_bad": int((~ok).sum())}


def buffered_counts(points, gene, rings, n_genes: int, dists, predicate: str = "contains", touched: int = 512,
                    small_genes: int = 2048) -> dict:
    """the oracle of segger_amd.buffered_counts.buffered_counts: numpy arrays under the product's names, ``counters`` in
    COUNTER_NAMES order.  ``touched`` and ``small_genes`` are SEGGER_BCOUNT_TOUCHED and SEGGER_BCOUNT_SMALL_GENES."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    P = len(rings)
    dists = np.broadcast_to(np.asarray(dists, dtype=np.float64), (P,))
    out = csr_from_pairs(pairs(points, rings, dists, predicate), gene, P, n_genes)
    row_len = np.diff(out["indptr"])
    n_ok_rings = sum(len(mc.open_ring(r)) >= 3 for r in rings)
    out["counters"] = np.array([out.pop("n_pairs"), len(out["indices"]), out.pop("n_bad"), int((row_len > touched).sum()),
                                n_ok_rings if n_genes > small_genes else 0], dtype=np.int64)
    return out


def dense(csr: dict, n_genes: int) -> np.ndarray:
    P = len(csr["indptr"]) - 1
    m = np.zeros((P, n_genes), dtype=np.int64)
    m[np.repeat(np.arange(P), np.diff(csr["indptr"])), csr["indices"]] = csr["counts"]
    return m


def from_dense(m: np.ndarray) -> dict:
    row, col = np.nonzero(m)
    indptr = np.zeros(m.shape[0] + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(row, minlength=m.shape[0]))
    return {"indptr": indptr, "indices": col.astype(np.int32), "counts": m[row, col].astype(np.int32), "cell_count": m.sum(1)}


def filter_boundaries(rings, inset, outset) -> np.ndarray:
    """the reference's keep rule, its arithmetic and its names: every test inclusive on both ends, over all stored vertices"""
    x2, y2, x3, y3 = inset
    x1, y1, x4, y4 = outset

    def between(v, lo, hi):
        return (v >= lo) & (v <= hi)

    keep = np.zeros(len(rings), dtype=bool)
    for p, r in enumerate(rings):
        r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
        x, y = r[:, 0], r[:, 1]
        center = int((between(x, x2, x3) & between(y, y2, y3)).sum())
        top = int((between(x, x1, x4) & between(y, y1, y2)).sum())
        left = int((between(x, x1, x2) & between(y, y1, y4)).sum())
        right = int((between(x, x3, x4) & between(y, y1, y4)).sum())
        bottom = int((between(x, x1, x4) & between(y, y3, y4)).sum())
        keep[p] = center == len(r) or (center > 0 and left > 0 and bottom == 0) or (center > 0 and top > 0 and right == 0)
    return keep


def buffered_counts_regions(points, gene, rings, n_genes: int, regions, dists, overlap: float, predicate: str = "contains") -> dict:
    """the sum over regions: strictly-inside points of the grown region, the kept polygons, the oracle on those"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    gene = np.asarray(gene)
    P = len(rings)
    dists = np.broadcast_to(np.asarray(dists, dtype=np.float64), (P,))
    total = np.zeros((P, n_genes), dtype=np.int64)
    kept = np.zeros(P, dtype=np.int64)
    n_pairs = n_bad = 0
    for xmin, ymin, xmax, ymax in np.asarray(regions, dtype=np.float64).reshape(-1, 4):
        outset = (xmin - overlap, ymin - overlap, xmax + overlap, ymax + overlap)
        keep = filter_boundaries(rings, (xmin, ymin, xmax, ymax), outset)
        kept += keep
        rows = np.flatnonzero(keep)
        sel = np.flatnonzero((points[:, 0] > outset[0]) & (points[:, 0] < outset[2]) & (points[:, 1] > outset[1]) & (points[:, 1] < outset[3]))
        if len(rows) == 0 or len(sel) == 0:
            continue
        sub = buffered_counts(points[sel], gene[sel], [rings[p] for p in rows], n_genes, dists[rows], predicate)
        total[rows] += dense(sub, n_genes)
        n_pairs += int(sub["counters"][0])
        n_bad += int(sub["counters"][2])
    out = from_dense(total)
    out["kept"] = kept
    out["n_pairs"], out["n_bad"] = n_pairs, n_bad
    return out


# ---------------------------------------------------------------- the scenes ---
def _q(a) -> np.ndarray:
    return mc.quantize(a)


def _square(x0, y0, side) -> np.ndarray:
    return np.array([[x0, y0], [x0 + side, y0], [x0 + side, y0 + side], [x0, y0 + side]], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def scene_routes(seed: int = 3) -> tuple:
    """rings of 3, 64, 65 and 4096 vertices (the register and the LDS ring route, at their edge and at the cap), 40 apart,
    about 250 points around each and one on a vertex of each -> (rings, points, gene), genes below 50"""
    rng = np.random.default_rng(seed)
    rings, pts = [], []
    for k, n in enumerate((3, 64, 65, 4096)):
        ring = mc.star_ring(n, 100 + n) + _q(ORIGIN + np.array([40.0 * k, 0.0]))
        rings.append(ring)
        pts.append(_q(ORIGIN + np.array([40.0 * k, 0.0]) + rng.uniform(-10.0, 10.0, (250, 2))))
        pts.append(ring[:1])
    points = np.concatenate(pts)
    return tuple(rings), points, rng.integers(0, 50, len(points))


@functools.lru_cache(maxsize=None)
def scene_clusters(seed: int = 5) -> tuple:
    """clusters of 1, 63, 64 and 65 points (each well inside one grid cell whatever the grid: 2^-6 across) on rows of their
    own, 30 apart, with empty cells between them: the spans the wave walks hold 0, 1, 63, 64 and 65 points.  One small square
    per cluster, one around an empty place, and one ring around everything"""
    rng = np.random.default_rng(seed)
    rings, pts = [], []
    for k, n in enumerate((1, 63, 64, 65)):
        c = _q(ORIGIN + np.array([30.0 * k, 30.0 * k]))
        pts.append(c + rng.integers(0, 32, (n, 2)) / 2048.0)
        rings.append(_square(c[0] - 1.0, c[1] - 1.0, 2.0))
    e = _q(ORIGIN + np.array([0.0, 90.0]))
    rings.append(_square(e[0] - 1.0, e[1] - 1.0, 2.0))                # no point anywhere near
    rings.append(_square(ORIGIN[0] - 5.0, ORIGIN[1] - 5.0, 110.0))
    points = np.concatenate(pts)
    return tuple(rings), points, rng.integers(0, 7, len(points))


@functools.lru_cache(maxsize=None)
def scene_field(n_points: int = 2000, per_row: int = 8, n_rows: int = 5, seed: int = 9) -> tuple:
    """a Voronoi-like field: per_row x n_rows (40) 13-vertex star rings about 12 across on a jittered 12.5-lattice (they
    overlap their neighbours once grown), either orientation, some closed, and n_points uniform points -> (rings, points)"""
    rng = np.random.default_rng(seed)
    rings = []
    for p in range(per_row * n_rows):
        centre = (np.array([p % per_row, p // per_row]) + 0.5) * 12.5 + rng.uniform(-1.5, 1.5, 2)
        ring = mc.star_ring(13, 500 + p, 7.0)
        if p % 2:
            ring = ring[::-1]
        if p % 3 == 0:
            ring = np.concatenate([ring, ring[:1]])
        rings.append(np.ascontiguousarray(ring + _q(ORIGIN + centre)))
    points = _q(ORIGIN + rng.uniform(-2.0, [per_row * 12.5 + 2.0, n_rows * 12.5 + 2.0], (n_points, 2)))
    return tuple(rings), points


def field_genes(n_genes: int, n_points: int = 2000, seed: int = 13) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, n_genes, n_points)


def scene_overflow(n_distinct: int) -> tuple:
    """three squares: one holding n_distinct points of n_distinct different genes (more than the touched list holds when
    the caller sizes it so), one whose 20 hits all share gene 3, one without a hit -> (rings, points, gene, n_genes)"""
    side = int(np.ceil(np.sqrt(n_distinct)))
    k = np.arange(n_distinct)
    a = _q(ORIGIN) + np.stack([k % side, k // side], axis=1) * 0.125 + 0.0625
    b = _q(ORIGIN + np.array([50.0, 0.0])) + np.stack([np.arange(20) * 0.25, np.full(20, 0.5)], axis=1) + 0.125
    rings = (_square(ORIGIN[0], ORIGIN[1], side * 0.125 + 0.125), _square(ORIGIN[0] + 50.0, ORIGIN[1], 6.0),
             _square(ORIGIN[0] + 100.0, ORIGIN[1], 6.0))
    return rings, np.concatenate([a, b]), np.concatenate([(k * 7919) % n_distinct, np.full(20, 3)]), n_distinct


REGION_GRID = tuple((x0, y0, x0 + 70.0, y0 + 52.5) for y0 in (ORIGIN[1] - 20.0, ORIGIN[1] + 32.5)
                    for x0 in (ORIGIN[0] - 20.0, ORIGIN[0] + 50.0))          # 2 x 2 over the field and a margin
REGION_OVERLAP = 16.0                                                  # more than a ring is across
