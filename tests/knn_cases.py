"""Inputs of the grid kNN tests (no GPU, plain numpy), their float64 reference, the one checker every GPU comparison
goes through, and the certificate that every input decides what it is meant to decide.

A case is ``{"points": float32 [n, 2], "queries": float32 [m, 2] or None (self query), "k", "max_dist", "grid", "dist"}``:
``grid`` is ``"python"`` (the case goes through ``segger_amd.neighbors.knn_grid``, which picks the grid) or an explicit
``(x0, y0, cell, nx, ny)`` handed to the C entry point ``segger_knn_grid``; ``dist`` False asks for no distance output.
``exact`` marks a case whose float32 arithmetic is exact (small integers); ``adversarial`` lists, for the cases built
against the ring walk, ``{"query", "p", "a", "r"}``: the row, the point P the walk must find although float32 binning
puts it into ring ``r + 1``, and the point A (or None) the walk would report in its place.

The reference is float64 brute force over the float32 coordinates with a STRICT ``max_dist`` (scipy's
``distance_upper_bound``).  :func:`check` is tie-robust: it compares sorted distances, recomputes every reported
neighbour's distance, and compares padding exactly, all entries, no exceptions.  That only decides anything if no input
sits on a knife edge, so :func:`certify` demands of every case that no pair lies within ``MARGIN`` (relative) of
``max_dist`` unless the arithmetic is exact, and of every adversarial row that the walk with the exact-arithmetic stop
rule (:func:`emulate_walk`, the kernel's float32 operations in numpy) reports something ``MARGIN`` away from the truth
while the walk with the float32-sound rule reports the truth.  ``MARGIN`` is ten times the checker's ``RTOL``: neither
the rounding of a squared distance nor the tolerance can hide or fake a failure.  A case that fails is rebuilt here,
never excused in a GPU test."""
import functools
import math

import numpy as np

from segger_amd.neighbors import grid_rule

F = np.float32
RTOL = 1e-6          # a subtraction, a square, an add and a square root are ~3 * 2^-24 = 1.8e-7 relative; x4 over that
MARGIN = 1e-5
K_CAPS = (8, 9, 16, 17, 32, 33, 64)                  # both sides of every compile-time capacity of the query kernel
LATTICE = ((1.0, 8), (2.0, 16), (5.0, 64))           # (max_dist, k); 5 brings the 3-4-5 ties
GRID_A = (-14.640592, 0.45952073)                    # (x0, cell) of the explicit grids of the stop_* cases
GRID_B = (-29.690655, 2.3746033)


def f32(x):
    return float(F(x))


# ------------------------------------------------------------------------------------------------- reference, checker
def reference(case):
    """-> (dist float64 [m, k] sorted, +inf = padding; ids int64 [m, k], n = padding).  Strict ``max_dist``."""
    pts = case["points"].astype(np.float64)
    qs = pts if case["queries"] is None else case["queries"].astype(np.float64)
    n, k = len(pts), case["k"]
    d_out = np.full((len(qs), k), np.inf)
    i_out = np.full((len(qs), k), n, dtype=np.int64)
    for s in range(0, len(qs), 512):
        d = np.hypot(qs[s:s + 512, None, 0] - pts[None, :, 0], qs[s:s + 512, None, 1] - pts[None, :, 1])
        d[~(d < case["max_dist"])] = np.inf
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        dd = np.take_along_axis(d, order, 1)
        d_out[s:s + 512, :order.shape[1]] = dd
        i_out[s:s + 512, :order.shape[1]] = np.where(np.isinf(dd), n, order)
    return d_out, i_out


def check(case, nbr, dist, ref_dist):
    """Assert that the kernel's ``nbr`` (and ``dist``, unless the case asked for none) is a right answer:
    (a) each row of dist equals the sorted reference row within RTOL; (b) so does the float64 distance recomputed from
    points[nbr]; (c) the ids of a row are distinct; (d) the padding mask is the reference's; (e) padding is
    (n_points, +inf).  Every entry is compared."""
    pts = case["points"].astype(np.float64)
    qs = pts if case["queries"] is None else case["queries"].astype(np.float64)
    n = len(pts)
    nbr = np.asarray(nbr)
    assert nbr.shape == ref_dist.shape and nbr.dtype == np.int32
    pad = np.isinf(ref_dist)
    assert ((nbr >= 0) & (nbr <= n)).all(), "neighbour id out of range"
    assert np.array_equal(nbr == n, pad), f"padding differs in {int(((nbr == n) != pad).sum())} entries"           # (d)
    safe = np.where(pad, 0, nbr)
    again = np.hypot(pts[safe, 0] - qs[:, None, 0], pts[safe, 1] - qs[:, None, 1])
    again[pad] = np.inf
    fin = ~pad
    err = np.abs(again[fin] - ref_dist[fin]) / np.maximum(ref_dist[fin], np.finfo(np.float64).tiny)
    err[again[fin] == ref_dist[fin]] = 0.0
    assert (err <= RTOL).all(), f"a reported neighbour is {err.max():.3e} (relative) off the reference distance"   # (b)
    ids = np.where(pad, -1 - np.arange(nbr.shape[1])[None, :], nbr)
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "a row names a point twice"                                          # (c)
    if case.get("dist", True):
        dist = np.asarray(dist)
        assert dist.shape == ref_dist.shape and dist.dtype == np.float32
        assert np.isposinf(dist[pad]).all(), "padding distance is not +inf"                                        # (e)
        got = dist[fin].astype(np.float64)
        err = np.abs(got - ref_dist[fin]) / np.maximum(ref_dist[fin], np.finfo(np.float64).tiny)
        err[got == ref_dist[fin]] = 0.0
        assert (err <= RTOL).all(), f"dist is {err.max():.3e} (relative) off the reference"                        # (a)
        err = np.abs(got - again[fin]) / np.maximum(again[fin], np.finfo(np.float64).tiny)
        err[got == again[fin]] = 0.0
        assert (err <= RTOL).all(), f"dist is {err.max():.3e} (relative) off the distance of the id beside it"     # (b)
    else:
        assert dist is None


# ------------------------------------------------------------------------------- the kernel's float32 walk, in numpy
def python_grid(case):
    """The (x0, y0, cell, nx, ny) ``knn_grid`` hands to the kernel for this case."""
    both = case["points"] if case["queries"] is None else np.concatenate([case["points"], case["queries"]])
    x0, y0 = (float(v) for v in both.min(0))
    x1, y1 = (float(v) for v in both.max(0))
    cell, nx, ny = grid_rule(x0, y0, x1, y1, len(case["points"]), case["max_dist"])
    return x0, y0, cell, nx, ny


def grid_of(case):
    return python_grid(case) if case["grid"] == "python" else case["grid"]


def cells_of(xy, grid):
    """floorf((p - x0) * inv_cell) clamped, in the kernel's float32 operations -> int64 [n, 2]."""
    x0, y0, cell, nx, ny = grid
    inv = F(1) / F(cell)
    with np.errstate(over="ignore", invalid="ignore"):
        cx = np.clip(np.floor((xy[:, 0] - F(x0)) * inv), 0, nx - 1).astype(np.int64)
        cy = np.clip(np.floor((xy[:, 1] - F(y0)) * inv), 0, ny - 1).astype(np.int64)
    return np.stack([cx, cy], 1)


def emulate_walk(case, row, sound, strict):
    """The query kernel's ring walk for one query -> (float32 squared distances [k], ids [k]; inf / n = padding).
    ``sound`` False is the stop rule of exact cell coordinates (reach = r * cell), True shrinks the reach by
    2^-20 * max(nx, ny) cells; ``strict`` False keeps a candidate at exactly ``max_dist``."""
    grid = grid_of(case)
    _, _, cell, nx, ny = grid
    pts = case["points"]
    q = (pts if case["queries"] is None else case["queries"])[row]
    n, k = len(pts), case["k"]
    pc, qc = cells_of(pts, grid), cells_of(q[None], grid)[0]
    ring = np.abs(pc - qc).max(1)
    dx, dy = pts[:, 0] - q[0], pts[:, 1] - q[1]
    cd = dx * dx + dy * dy                                             # float32 throughout
    max_d2 = F(case["max_dist"]) * F(case["max_dist"])
    keep = (cd < max_d2) if strict else (cd <= max_d2)
    slack = F(math.ldexp(float(F(max(nx, ny))), -20)) if sound else F(0)

    def stops(r, kth):
        reach = max(F(r) - slack, F(0)) * F(cell)
        reach2 = reach * reach
        return reach2 >= max_d2 or kth <= reach2

    best_d, best_i = np.full(k, np.inf, dtype=F), np.full(k, n, dtype=np.int64)
    rmax = max(qc[0], nx - 1 - qc[0], qc[1], ny - 1 - qc[1])
    for r in np.unique(ring):                                          # the stop test is monotone in r between rings
        if r > rmax or (r > 0 and stops(r - 1, best_d[k - 1])):
            break
        sel = np.flatnonzero((ring == r) & keep)
        d_all, i_all = np.concatenate([best_d, cd[sel]]), np.concatenate([best_i, sel])
        order = np.argsort(d_all, kind="stable")[:k]
        best_d, best_i = d_all[order], i_all[order]
    return best_d, best_i


# ----------------------------------------------------------------------------------------------- the certificate
def near_max_dist(case):
    """The smallest |d - max_dist| / max_dist over every (query, point) pair, float64 (inf without a bound)."""
    if not math.isfinite(case["max_dist"]):
        return math.inf
    pts = case["points"].astype(np.float64)
    qs = pts if case["queries"] is None else case["queries"].astype(np.float64)
    worst = math.inf
    for s in range(0, len(qs), 512):
        d = np.hypot(qs[s:s + 512, None, 0] - pts[None, :, 0], qs[s:s + 512, None, 1] - pts[None, :, 1])
        worst = min(worst, float(np.abs(d - case["max_dist"]).min()) / case["max_dist"])
    return worst


def certify(case):
    """Assert the conditions of the module docstring; -> the smallest relative gap the case relies on (inf if none)."""
    pts, qs = case["points"], case["queries"]
    assert pts.dtype == F and pts.ndim == 2 and pts.shape[1] == 2 and np.isfinite(pts).all()
    assert qs is None or (qs.dtype == F and qs.ndim == 2 and qs.shape[1] == 2 and np.isfinite(qs).all())
    assert 1 <= case["k"] <= 64 and case["max_dist"] > 0 and case["max_dist"] == f32(case["max_dist"])
    assert len(pts) <= 5000 and (qs is None or len(qs) <= 5000)
    x0, y0, cell, nx, ny = grid_of(case)
    assert nx >= 1 and ny >= 1 and nx * ny < 2 ** 31 and cell > 0
    if case["grid"] == "python":                                       # what grid_rule promises
        n = len(pts)
        assert nx * ny <= 4 * n + nx + ny and max(nx, ny) <= 30001, (nx, ny, n)     # (a + 1)(b + 1), a * b <= 4n
        if max(nx, ny) <= 4 * min(nx, ny):                             # a box that is no strip: 4n + O(sqrt n)
            assert nx * ny <= 4 * n + 10 * math.sqrt(n) + 4, (nx, ny, n)
    gap = math.inf
    if case.get("exact"):                                              # small integers: every float32 operation is exact
        both = pts if qs is None else np.concatenate([pts, qs])
        assert np.array_equal(both, np.round(both)) and np.abs(both).max() < 1024 and case["max_dist"] < 1024
    else:
        gap = near_max_dist(case)
        assert gap >= MARGIN, f"a pair lies {gap:.3e} (relative) from max_dist"
    if case.get("adversarial"):
        ref_d, ref_i = reference(case)
        grid = grid_of(case)
        qall = pts if qs is None else qs
        max_d2 = F(case["max_dist"]) * F(case["max_dist"])
        for adv in case["adversarial"]:
            row, p, a, r = adv["query"], adv["p"], adv["a"], adv["r"]
            assert np.abs(cells_of(pts[p:p + 1], grid)[0] - cells_of(qall[row:row + 1], grid)[0]).max() == r + 1
            dq = pts[p] - qall[row]
            cd = dq[0] * dq[0] + dq[1] * dq[1]                         # float32, as the kernel has it
            reach2 = (F(r) * F(cell)) * (F(r) * F(cell))
            assert cd < reach2 and cd < max_d2, "P is not strictly inside the reach in the kernel's own arithmetic"
            d_p = float(np.hypot(*(pts[p].astype(np.float64) - qall[row].astype(np.float64))))
            gap = min(gap, 1.0 - d_p / (r * f32(cell)))
            assert p in ref_i[row], "the reference does not report P"
            bad_d, bad_i = emulate_walk(case, row, sound=False, strict=True)
            good_d, good_i = emulate_walk(case, row, sound=True, strict=True)
            assert p not in bad_i and p in good_i, "the walk over exact cells finds P, or the sound walk misses it"
            assert np.array_equal(np.sort(good_i), np.sort(ref_i[row])), "the sound walk differs from brute force"
            if a is None:                                              # finite max_dist: the row comes back short
                assert math.isfinite(case["max_dist"]) and (bad_i == len(pts)).sum() == np.isinf(ref_d[row]).sum() + 1
                gap = min(gap, 1.0 - d_p / case["max_dist"])
            else:                                                      # the row comes back with A in P's place
                da = (pts[a] - qall[row]).astype(np.float64)
                d_a = float(np.hypot(*da))
                assert a in bad_i and a not in ref_i[row] and d_p < d_a <= r * f32(cell)
                kth = np.sqrt(bad_d.astype(np.float64))[-1]
                assert abs(kth - d_a) <= RTOL * d_a and ref_d[row, -1] == d_p, "A and P are not the two k-th distances"
                gap = min(gap, d_a / d_p - 1.0)
    if case.get("inclusive_differs"):                                  # an inclusive bound must change the answer
        ref_d, _ = reference(case)
        rows = [i for i in range(len(ref_d)) if np.isinf(ref_d[i]).any()][:8]
        assert rows and any((emulate_walk(case, i, sound=True, strict=False)[1] != len(pts)).sum() > np.isfinite(ref_d[i]).sum()
                            for i in rows)
    return gap


# ------------------------------------------------------------------------------------ float32 search for ring skips
def ring_skips(x0, cell, r, sgn, lo=3000, hi=29000, min_gap=4e-5):
    """Abscissae (q, p) with |p - q| < r * cell in float32, although floorf((. - x0) * (1 / cell)) puts p exactly r + 1
    cells from q (to the right for sgn = +1).  Directed search: for every cell j the last float32 number of the cell, paired
    with the first one of the cell r + 1 farther (true distance: r cells and a rounding).  -> (q, p, relative gap 1 - |p - q| / (r * cell)),
    largest gap first."""
    x0, cell = F(x0), F(cell)
    inv = F(1) / cell

    def t(x):
        return np.floor((x - x0) * inv)

    def first_in(j):                                                   # the smallest float32 whose cell is >= j
        x = (np.float64(x0) + j * np.float64(cell)).astype(F)
        for _ in range(48):
            x = np.where(t(x) >= j, np.nextafter(x, F(-np.inf)), x).astype(F)
        for _ in range(49):
            x = np.where(t(x) < j, np.nextafter(x, F(np.inf)), x).astype(F)
        assert (t(x) >= j).all() and (t(np.nextafter(x, F(-np.inf))) < j).all()
        return x

    j = np.arange(lo, hi, dtype=np.float64)
    if sgn > 0:                                                        # q at the top of cell j, p at the bottom of j + r + 1
        q, p = np.nextafter(first_in(j + 1), F(-np.inf)), first_in(j + r + 1)
    else:
        q, p = first_in(j), np.nextafter(first_in(j - r), F(-np.inf))
    assert (np.abs(t(p) - t(q)) == r + 1).all()
    d = np.abs(p - q)                                                  # float32, as the kernel subtracts
    reach = F(r) * cell
    gap = 1.0 - d.astype(np.float64) / float(reach)
    ok = np.flatnonzero((d * d < reach * reach) & (gap >= min_gap))
    ok = ok[np.argsort(-gap[ok], kind="stable")]
    return q[ok], p[ok], gap[ok]


def spread(q, p, count, apart):
    """The first ``count`` pairs (largest gaps first) whose queries are at least ``apart`` from one another."""
    taken = []
    for i in range(len(q)):
        if all(abs(float(q[i]) - float(q[j])) >= apart for j in taken):
            taken.append(i)
        if len(taken) == count:
            return q[taken], p[taken]
    raise AssertionError(f"only {len(taken)} of {count} pairs found")


def swap_axes(case):
    out = dict(case)
    out["points"] = np.ascontiguousarray(case["points"][:, ::-1])
    out["queries"] = None if case["queries"] is None else np.ascontiguousarray(case["queries"][:, ::-1])
    x0, y0, cell, nx, ny = case["grid"]
    out["grid"] = (y0, x0, cell, ny, nx)
    return out


def stop_case(grid_xc, r, k, bounded, seed):
    """Separate queries on the explicit grid (x0, 0, cell, 30001, 8 per query); per query: P in ring r + 1 yet nearer than
    r * cell (``ring_skips``, both directions in x), k - 1 points close by and, without a bound, A above the query at a
    distance half way between P's and r * cell, where it is the k-th neighbour for the walk that stops after ring r.
    ``bounded`` sets max_dist = cell (r must be 1): the walk then stops after ring 1 and the row comes back short."""
    x0, cell = f32(grid_xc[0]), f32(grid_xc[1])
    rng = np.random.default_rng(seed)
    pts, qs, adv = [], [], []
    for sgn in (1, -1):
        qx, px = spread(*ring_skips(x0, cell, r, sgn)[:2], count=3 if r == 1 else 2, apart=(r + 3) * cell)
        for a, b in zip(qx, px):
            qy = F((8 * len(qs) + 0.3) * cell)                         # a band of rows of its own: a pair read backwards
            row = len(qs)                                              # is a pair of the other direction
            qs.append((a, qy))
            adv.append({"query": row, "p": len(pts), "a": None, "r": r})
            pts.append((b, qy))
            for i in range(k - 1):                                     # the nearer neighbours of the row
                pts.append((a, F(qy + (0.05 + 0.07 * i) * cell)))
            if not bounded:
                d_p = abs(float(b) - float(a))
                adv[-1]["a"] = len(pts)
                pts.append((a, F(float(qy) + 0.5 * (d_p + r * cell))))
    ny = 8 * len(qs)
    filler = np.stack([rng.uniform(x0, x0 + 30000 * cell, 60), rng.uniform(0, ny * cell, 60)], 1)
    qarr = np.array(qs, dtype=F)
    filler = filler[np.abs(filler[:, None, 0] - qarr[None, :, 0].astype(np.float64)).min(1) > 8 * cell]
    return {"points": np.concatenate([np.array(pts, dtype=F), filler.astype(F)]), "queries": qarr, "k": k,
            "max_dist": cell if bounded else math.inf, "grid": (x0, 0.0, cell, 30001, ny), "adversarial": adv}


def stop_python_case():
    """The bounded kind through ``knn_grid``: a strip 9000 wide and 0.3 high, n = 4000 and a max_dist for which the grid
    rule itself picks cell == max_dist, nx ~ 20000, ny = 1; self query."""
    x0, cell = f32(GRID_A[0]), f32(GRID_A[1])
    width, height, n = 9000.0, 0.3, 4000
    rng = np.random.default_rng(5)
    pts, adv = [(F(x0), F(0)), (F(x0 + width), F(height))], []        # the corners fix the bounding box
    qx, px = spread(*ring_skips(x0, cell, 1, 1, lo=3000, hi=int(width / cell) - 10)[:2], count=3, apart=4 * cell)
    for a, b in zip(qx, px):
        adv.append({"query": len(pts), "p": len(pts) + 1, "a": None, "r": 1})
        adv.append({"query": len(pts) + 1, "p": len(pts), "a": None, "r": 1})          # a self query sees it both ways
        pts += [(a, F(0.25)), (b, F(0.25))]
    special = np.array(pts, dtype=F)
    filler = np.stack([rng.uniform(x0, x0 + width, 2 * n), rng.uniform(0, height, 2 * n)], 1)
    filler = filler[np.abs(filler[:, None, 0] - special[None, 2:, 0].astype(np.float64)).min(1) > 4 * cell]
    points = np.concatenate([special, filler[:n - len(special)].astype(F)])
    return {"points": points, "queries": None, "k": 8, "max_dist": cell, "grid": "python", "adversarial": adv}


# ------------------------------------------------------------------------------------------------------- the cases
def clustered(rng, n, lo=0.0, hi=100.0, sigma=2.0):
    centres = rng.uniform(lo, hi, size=(max(n // 50, 1), 2))
    return (centres[rng.integers(0, len(centres), n)] + rng.normal(0, sigma, size=(n, 2))).astype(F)


def case(points, queries=None, k=8, max_dist=math.inf, grid="python", **more):
    return dict({"points": np.ascontiguousarray(points, dtype=F),
                 "queries": None if queries is None else np.ascontiguousarray(queries, dtype=F),
                 "k": k, "max_dist": f32(max_dist), "grid": grid}, **more)


def lattice_cases():
    xy = np.stack(np.meshgrid(np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 2)
    out = {}
    for max_dist, k in LATTICE:
        out[f"lattice_strict_d{int(max_dist)}_k{k}"] = case(xy, k=k, max_dist=max_dist, exact=True, inclusive_differs=True)
        out[f"lattice_strict_d{int(max_dist)}_k{k}_abi"] = case(xy, k=k, max_dist=max_dist, grid=(-0.25, -0.75, 1.5, 9, 9),
                                                               exact=True, inclusive_differs=True)
    return out


def k_caps_cases():
    rng = np.random.default_rng(300)
    big, small = clustered(rng, 300), clustered(rng, 20, sigma=4.0)
    out = {}
    for k in K_CAPS:
        out[f"k_caps_n300_k{k}"] = case(big, k=k)
        out[f"k_caps_n20_k{k}"] = case(small, k=k)                      # n < k for the large ones: the padding tail
    return out


def degenerate_cases():
    rng = np.random.default_rng(77)
    out = {}

    def both(name, points, queries, **kw):
        out[f"degenerate_{name}_self"] = case(points, **kw)
        out[f"degenerate_{name}_query"] = case(points, queries, **kw)

    ring = np.array([(math.cos(a), math.sin(a)) for a in np.linspace(0, 6, 16)])
    both("coincident", np.tile([(3.0, 4.0)], (500, 1)), np.concatenate([[(3.0, 4.0)], (3.0, 4.0) + 0.75 * ring]), k=6)
    far = (8191.5, 16383.25)
    both("coincident_far", np.tile([far], (500, 1)), np.concatenate([[far], np.array(far) + 0.25 * np.round(4 * ring)]), k=6)
    clumps = np.concatenate([np.tile([(0.0, 0.0)], (40, 1)), np.tile([(600.0, 800.0)], (40, 1))])     # 1000 apart, exactly
    both("two_clumps", clumps, [(0, 0), (600, 800), (300, 401), (-50, 7), (650, 790)], k=64)
    x = np.sort(rng.uniform(0, 100, 300))
    both("horizontal_line", np.stack([x, np.full(300, 7.25)], 1), np.stack([rng.uniform(-5, 105, 40), np.full(40, 7.25)], 1))
    both("vertical_line", np.stack([np.full(300, -3.5), x], 1), np.stack([rng.uniform(-4, -3, 40), rng.uniform(-5, 105, 40)], 1))
    one = [(2.5, -1.5)]
    both("n1_k1", one, [(2.5, -1.5), (0, 0), (100, 100)], k=1)
    both("n1_k5", one, [(2.5, -1.5), (0, 0), (100, 100)], k=5)
    both("n2", [(0.0, 0.0), (3.0, 4.0)], [(0, 0), (1.5, 2.1), (3, 4), (-7, 9)], k=3)
    both("duplicates_x4", np.repeat(clustered(rng, 250), 4, axis=0), clustered(rng, 60), k=6)
    crowd = np.concatenate([rng.uniform(0, 50, (1999, 2)), [(1e6, 1e6)]])
    both("outlier_one_cell", crowd, np.concatenate([rng.uniform(-5, 55, (60, 2)), [(1e6, 1e6), (5e5, 5e5)]]), k=8)
    both("negative", clustered(rng, 400, lo=-300.0, hi=-100.0), rng.uniform(-310, -90, (80, 2)), k=8, max_dist=2.7)
    return out


def abi_grid_cases():
    rng = np.random.default_rng(400)
    pts, qs = clustered(rng, 400), rng.uniform(-5, 105, (100, 2)).astype(F)
    lo = float(min(pts.min(), qs.min())) - 1.0
    hi = float(max(pts.max(), qs.max())) + 1.0
    span = hi - lo
    grids = {"one_cell": (lo, lo, span, 1, 1),
             "coarse": (lo, lo, 10 * math.sqrt(span * span * 2 / 400), 2, 2),
             "fine": (lo, lo, span / 500, 501, 501),
             "middle_third": (lo + span / 3, lo + span / 3, 4.0, int(span / 12) + 1, int(span / 12) + 1),
             "off_grid": (hi + 10.0, lo, 4.0, 8, int(span / 4) + 1)}
    out = {}
    for name, grid in grids.items():
        grid = tuple(f32(v) if i < 3 else v for i, v in enumerate(grid))
        out[f"abi_grids_{name}"] = case(pts, qs, k=8, grid=grid)
        out[f"abi_grids_{name}_self_bounded"] = case(pts, None, k=8, max_dist=2.7, grid=grid)       # queries == NULL
        out[f"abi_grids_{name}_no_dist"] = case(pts, qs, k=8, max_dist=2.7, grid=grid, dist=False)  # dist == NULL
    return out


def stop_cases():
    out = {"stop_maxdist_x": stop_case(GRID_A, 1, 4, True, 1), "stop_maxdist_x_wide_cell": stop_case(GRID_B, 1, 4, True, 2)}
    out["stop_maxdist_y"] = swap_axes(out["stop_maxdist_x"])
    for k in (1, 3):
        for r in (1, 2):
            out[f"stop_kth_k{k}_r{r}"] = stop_case(GRID_A if r == 1 else GRID_B, r, k, False, 10 * k + r)
    out["stop_kth_k3_r1_y"] = swap_axes(out["stop_kth_k3_r1"])
    out["stop_python_grid"] = stop_python_case()
    return out


NAMES = ([f"lattice_strict_d{int(d)}_k{k}{s}" for d, k in LATTICE for s in ("", "_abi")]
         + ["stop_maxdist_x", "stop_maxdist_x_wide_cell", "stop_maxdist_y", "stop_kth_k1_r1", "stop_kth_k1_r2", "stop_kth_k3_r1",
            "stop_kth_k3_r2", "stop_kth_k3_r1_y", "stop_python_grid"]
         + [f"k_caps_n{n}_k{k}" for k in K_CAPS for n in (300, 20)]
         + [f"degenerate_{d}_{s}" for d in ("coincident", "coincident_far", "two_clumps", "horizontal_line", "vertical_line", "n1_k1",
                                            "n1_k5", "n2", "duplicates_x4", "outlier_one_cell", "negative") for s in ("self", "query")]
         + [f"abi_grids_{g}{s}" for g in ("one_cell", "coarse", "fine", "middle_third", "off_grid")
            for s in ("", "_self_bounded", "_no_dist")])


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> case, in the order of ``NAMES`` (the parametrisation of the tests); built once per process."""
    cases = {}
    for part in (lattice_cases, stop_cases, k_caps_cases, degenerate_cases, abi_grid_cases):
        cases.update(part())
    assert sorted(cases) == sorted(NAMES)
    return {name: cases[name] for name in NAMES}


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """The float64 reference of a case, computed once and shared (read-only) by the tests that need it."""
    d, i = reference(all_cases()[name])
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i
