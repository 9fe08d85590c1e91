"""The oracle and the cases of the ring-rasterisation tests (plain numpy and the standard library: no product import).

The contract (include/segger_amd.h, "Ring rasterisation"): the pixel in row r, column c stands for the world point
(c sx + tx, r sy + ty), one multiplication and one addition in float64, not fused; it belongs to polygon p when that point
satisfies the join's predicate at distance 0 against ring p.  The oracle therefore IMPORTS the join's oracles from
polygon_join_cases.py and copies nothing: ``match_f64`` (float64, translated to the ring's first vertex) over the pixel
centres, and ``pair_exact`` (integers) to pin the candidate set.  The pixel centres are ``np.arange(n) * s + t``, two numpy
operations, so they are the device's bits.

The exact oracle: every float64 is an integer multiple of a power of two, so a ring and the pixel centres are scaled by one
power of two into Python integers and handed to ``pair_exact``; at distance 0 only the parity and whether dist2 is zero
matter, and both are scale-free.

Overlaps: a pixel matched by several polygons goes to the lowest or the highest polygon INDEX; the label is read afterwards.
"""
import functools
from fractions import Fraction

import numpy as np

import contour_cases as cc
import morphology_cases as mc
import polygon_join_cases as pc

PREDICATES = ("contains", "intersects")
OVERLAPS = ("lowest", "highest")
COUNTER_NAMES = ("n_pixels_set", "n_overlaps", "n_empty", "n_clipped", "n_degenerate", "n_large_tier", "n_blocks_filled")
PINNED = COUNTER_NAMES[:6]           # n_blocks_filled is the device's own diagnostic: it depends on the block side
CHUNK = 2048                         # pixel centres per call of match_f64 (it builds [points, edges] arrays)


def centres(shape, scale, translation):
    """(X [W], Y [H]): the world coordinates of the pixel centres, as the device computes them"""
    H, W = shape
    X = np.arange(W, dtype=np.float64) * np.float64(scale[0]) + np.float64(translation[0])
    Y = np.arange(H, dtype=np.float64) * np.float64(scale[1]) + np.float64(translation[1])
    return X, Y


def _candidates(ring, X, Y, grow):
    """(rows, cols) of the pixels whose centre is within the ring's bounds grown by ``grow`` (exact comparisons)"""
    r = mc.open_ring(ring)
    cols = np.flatnonzero((X >= r[:, 0].min() - grow) & (X <= r[:, 0].max() + grow))
    rows = np.flatnonzero((Y >= r[:, 1].min() - grow) & (Y <= r[:, 1].max() + grow))
    rr, kk = np.meshgrid(rows, cols, indexing="ij")
    return rr.ravel(), kk.ravel()


def masks_f64(rings, shape, scale=(1.0, 1.0), translation=(0.0, 0.0)):
    """per polygon {"contains": flat pixel indices, "intersects": ...} from the join's float64 oracle.  Every pixel within the
    bounds grown by two pixels is asked: the predicate decides, not the box."""
    H, W = shape
    X, Y = centres(shape, scale, translation)
    grow = 2.0 * (abs(scale[0]) + abs(scale[1]))
    out = []
    for ring in rings:
        if len(mc.open_ring(ring)) < 3:
            out.append({name: np.zeros(0, np.int64) for name in PREDICATES})
            continue
        rows, cols = _candidates(ring, X, Y, grow)
        con, inter = [], []
        for k in range(0, len(rows), CHUNK):
            pts = np.stack([X[cols[k:k + CHUNK]], Y[rows[k:k + CHUNK]]], axis=1)
            c, i, _, _ = pc.match_f64(pts, ring, 0.0)
            con.append(c)
            inter.append(i)
        con = np.concatenate(con + [np.zeros(0, bool)])
        inter = np.concatenate(inter + [np.zeros(0, bool)])
        flat = rows.astype(np.int64) * W + cols
        out.append({"contains": np.sort(flat[con]), "intersects": np.sort(flat[inter])})
    return out


def _scaled_ints(values, den):
    return [int(Fraction(float(v)) * den) for v in values]


def masks_exact(rings, shape, scale=(1.0, 1.0), translation=(0.0, 0.0)):
    """the same from ``polygon_join_cases.pair_exact`` on integers: the exact-rational predicate of that file.  Outside the
    ring's bounds nothing matches (no edge straddles the point and dist2 > 0), so only the pixels inside them are asked."""
    H, W = shape
    X, Y = centres(shape, scale, translation)
    out = []
    for ring in rings:
        r = mc.open_ring(ring)
        if len(r) < 3:
            out.append({name: np.zeros(0, np.int64) for name in PREDICATES})
            continue
        rows, cols = _candidates(ring, X, Y, 0.0)
        used = np.concatenate([r.ravel(), X[np.unique(cols)], Y[np.unique(rows)]])
        den = max(Fraction(float(v)).denominator for v in used)      # powers of two: the largest is a common one
        xi = dict(zip(np.unique(cols).tolist(), _scaled_ints(X[np.unique(cols)], den)))
        yi = dict(zip(np.unique(rows).tolist(), _scaled_ints(Y[np.unique(rows)], den)))
        iring = list(zip(_scaled_ints(r[:, 0], den), _scaled_ints(r[:, 1], den)))
        con, inter = [], []
        for row, col in zip(rows.tolist(), cols.tolist()):
            parity, dist2 = pc.pair_exact((xi[col], yi[row]), iring)
            if parity and dist2 > 0:
                con.append(row * W + col)
            if parity or dist2 == 0:
                inter.append(row * W + col)
        out.append({"contains": np.asarray(sorted(con), np.int64), "intersects": np.asarray(sorted(inter), np.int64)})
    return out


def clipped(ring, shape, scale, translation):
    """do the ring's bounds leave the closed rectangle of the pixel centres?"""
    X, Y = centres(shape, scale, translation)
    r = mc.open_ring(ring)
    return bool(r[:, 0].min() < min(X[0], X[-1]) or r[:, 0].max() > max(X[0], X[-1]) or
                r[:, 1].min() < min(Y[0], Y[-1]) or r[:, 1].max() > max(Y[0], Y[-1]))


def resolve(masks, rings, shape, scale, translation, labels, predicate, overlap):
    """the image, the per-polygon counts and the pinned counters from the per-polygon masks"""
    H, W = shape
    P = len(rings)
    owner = np.full(H * W, -1, np.int64)
    order = range(P - 1, -1, -1) if overlap == "lowest" else range(P)        # the last writer wins
    for p in order:
        owner[masks[p][predicate]] = p
    lab = np.arange(1, P + 1, dtype=np.int32) if labels is None else np.asarray(labels, np.int32)
    image = np.where(owner >= 0, lab[np.maximum(owner, 0)] if P else 0, 0).astype(np.int32).reshape(H, W)
    n_covered = np.asarray([len(masks[p][predicate]) for p in range(P)], np.int64)
    n_won = np.bincount(owner[owner >= 0], minlength=P).astype(np.int64)
    real = [len(mc.open_ring(r)) >= 3 for r in rings]
    counters = {"n_pixels_set": int((owner >= 0).sum()), "n_overlaps": int(n_covered.sum() - (owner >= 0).sum()),
                "n_empty": int((n_covered == 0).sum()),
                "n_clipped": sum(clipped(r, shape, scale, translation) for r, ok in zip(rings, real) if ok),
                "n_degenerate": P - sum(real),
                "n_large_tier": sum(len(mc.open_ring(r)) > 64 for r in rings)}
    return {"image": image, "n_covered": n_covered, "n_won": n_won, "counters": counters}


# ---------------------------------------------------------------- the cases ---
def _rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


def case(name, rings, shape, scale=(1.0, 1.0), translation=(0.0, 0.0), labels=None):
    return {"name": name, "rings": [np.asarray(r, np.float64).reshape(-1, 2) for r in rings], "shape": shape, "scale": scale,
            "translation": translation, "labels": labels}


HAND_SQUARE = _rect(1, 1, 3, 3)
HAND_TRIANGLE = np.array([[4.0, 4.0], [7.0, 4.0], [4.0, 7.0]])


def hand_image(predicate):
    """worked by hand: the square's closed set is the 9 lattice points of [1, 3]^2, its open set (2, 2) alone; the
    triangle's closed set is x >= 4, y >= 4, x + y <= 11 (10 points), its open set (5, 5) alone"""
    img = np.zeros((8, 8), np.int32)
    if predicate == "intersects":
        img[1:4, 1:4] = 1
        for y in range(4, 8):
            img[y, 4:12 - y] = 2
    else:
        img[2, 2] = 1
        img[5, 5] = 2
    return img


def widths(block):
    """rectangles 1, 61 .. 65 and block - 3 .. block + 1 pixel columns wide (the walk widens a range by a pixel on each
    side, so the walked widths reach 63, 64, 65 and block - 1, block, block + 1 as well), two rows each"""
    ws = sorted({1, 61, 62, 63, 64, 65} | set(range(max(block - 3, 1), block + 2)))
    return [_rect(2.75, 1.5 + 4 * k, 2.75 + w - 0.5, 3.5 + 4 * k) for k, w in enumerate(ws)], ws


@functools.lru_cache(maxsize=None)
def scene_image():
    """the 128 x 128 Voronoi scene of the GPU tests (another seeded scene of contour_cases.voronoi)"""
    return cc.voronoi(128, 48, 9.0, 7)


@functools.lru_cache(maxsize=None)
def scene():
    """(image, cc.expected(image), admitted labels) of the scene, computed once"""
    img = scene_image()
    want = cc.expected(img)
    return img, want, tuple(cc.admitted(img, want["by_label"]))


def rings_of(want, only=None):
    """the rings of cc.expected's result as a list (``only``: these labels), and their labels"""
    ids = want["label_ids"].tolist()
    keep = [k for k, lab in enumerate(ids) if only is None or lab in only]
    offs, xy = want["ring_offsets"], want["xy"]
    return [xy[offs[k]:offs[k + 1]] for k in keep], np.asarray([ids[k] for k in keep], np.int32)


@functools.lru_cache(maxsize=None)
def cases(block=8):
    sq = _rect(0, 0, 1, 1)
    out = [
        case("hand8", [HAND_SQUARE, HAND_TRIANGLE], (8, 8)),
        case("tier_edges", [mc.star_ring(3, 1, 7.0) + [9.0, 9.0], mc.star_ring(64, 2, 7.0) + [22.0, 9.0],
                            mc.star_ring(65, 3, 7.0) + [9.0, 22.0], (mc.star_ring(64, 4, 7.0) + [22.0, 22.0])[::-1]], (32, 32)),
        case("ring4096", [mc.star_ring(4096, 5, 7.0) + [8.0, 8.0]], (16, 16)),
        case("widths", widths(block)[0], (4 * len(widths(block)[1]) + 2, 72)),
        case("one_column", [_rect(-3.0, 1.5, 4.0, 5.5)], (9, 1)),
        case("one_row", [_rect(1.5, -2.0, 70.5, 2.0)], (1, 80)),
        case("outside_and_clipped", [_rect(20.0, 20.0, 25.0, 25.0), _rect(-3.5, 4.0, 2.5, 7.0), _rect(12.5, 4.0, 19.0, 7.0),
                                     _rect(5.0, -4.0, 8.0, 1.5), _rect(5.0, 13.5, 8.0, 22.0), _rect(-5.0, -5.0, 30.0, 30.0)], (16, 16)),
        case("sliver", [_rect(2.25, 1.0, 2.75, 6.0)], (8, 8)),
        case("collinear", [np.array([[1.0, 1.0], [3.0, 3.0], [5.0, 5.0]]), np.array([[1.0, 6.0], [5.0, 6.0], [3.0, 6.0], [2.0, 6.0]])], (8, 8)),
        case("degenerate", [np.zeros((0, 2)), np.array([[2.0, 2.0]]), np.array([[1.0, 1.0], [4.0, 4.0]]),
                            np.array([[1.0, 1.0], [4.0, 4.0], [1.0, 1.0]]), _rect(2, 2, 5, 5)], (8, 8)),
        case("nested_twins_shared_edge", [_rect(1, 1, 12, 12), _rect(3, 3, 8, 8), _rect(3, 3, 8, 8)[::-1], _rect(12, 1, 18, 12),
                                          np.concatenate([_rect(5, 5, 6, 6), _rect(5, 5, 6, 6)[:1]])], (14, 20)),
        case("flipped_y", [mc.star_ring(13, 6, 6.0) + [108.5, -57.25], mc.star_ring(25, 7, 5.0) + [115.0, -60.0]], (24, 28),
             scale=(1.0, -1.0), translation=(100.5, -48.25)),
        case("scale_0.2125", [mc.star_ring(13, 8, 3.0) + [5004.0, 7003.5], mc.star_ring(70, 9, 2.5) + [5007.0, 7005.0]], (40, 48),
             scale=(0.2125, 0.2125), translation=(5000.0, 7000.0)),
        case("scale_anisotropic_negative_x", [mc.star_ring(20, 10, 4.0) + [-3.0, 6.0]], (30, 34), scale=(-0.5, 0.375),
             translation=(2.0, 1.0)),
    ]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name, block=8):
    """the float64 masks of a case, computed once per process"""
    c = next(c for c in cases(block) if c["name"] == name)
    return masks_f64(c["rings"], c["shape"], c["scale"], c["translation"])


def expected(c, predicate, overlap, masks=None, block=8):
    masks = reference(c["name"], block) if masks is None else masks
    return resolve(masks, c["rings"], c["shape"], c["scale"], c["translation"], c["labels"], predicate, overlap)
