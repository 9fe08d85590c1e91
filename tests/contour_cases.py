"""The oracle and the cases of the label-contour tests (no GPU, numpy only).

The oracle is a sequential Suzuki-Abe border following written from the contract in include/segger_amd.h: a raster scan
that starts an outer border at a pixel with background before it and a hole border at a pixel with background after it,
follows it with the clockwise / counter-clockwise neighbour search of the paper, and MARKS the pixels (NBD, -NBD) so that no
border is followed twice.  The device code has no marks and no sequential scan (it follows every border from candidate
pixels in parallel and keeps the walk that started lowest), so the two share the definition and nothing else.  On top of it:
CHAIN_APPROX_SIMPLE from coordinate differences, the canonical start, the selection and the tie rule.

The frame is the reference's: it hands cv2 the TRANSPOSED crop, so "rows" are x and "columns" are y and the scan is
x-major.  Images here are [H, W] with row = y, column = x; rings are (x, y)."""
import numpy as np

# neighbours clockwise on the screen of the transposed crop (rows = x down, columns = y right), from "y - 1"
CW = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]
CW_INDEX = {d: k for k, d in enumerate(CW)}
MORPH_MAX_VERTS = 4096
LDS_BITS = 32768


def borders(fg):
    """Every border of the boolean image ``fg`` [n_x, n_y] (rows = x), each once: a list of chains; a chain is the list of
    its states (x, y, clockwise code of the previous pixel or None for an isolated pixel) in the order of travel."""
    nx, ny = fg.shape
    f = np.zeros((nx + 2, ny + 2), np.int64)
    f[1:-1, 1:-1] = fg
    nbd, out = 1, []
    for i in range(1, nx + 1):
        for j in range(1, ny + 1):
            if f[i, j] == 1 and f[i, j - 1] == 0:
                i2, j2 = i, j - 1
            elif f[i, j] >= 1 and f[i, j + 1] == 0:
                i2, j2 = i, j + 1
            else:
                continue
            nbd += 1
            k0 = CW_INDEX[(i2 - i, j2 - j)]
            first = None
            for k in range(1, 8):                                    # (3.1) clockwise from the background pixel
                d = CW[(k0 + k) % 8]
                if f[i + d[0], j + d[1]] != 0:
                    first = (i + d[0], j + d[1])
                    break
            if first is None:
                f[i, j] = -nbd
                out.append([(i - 1, j - 1, None)])
                continue
            (i2, j2), (i3, j3) = first, (i, j)
            chain = []
            while True:
                k2 = CW_INDEX[(i2 - i3, j2 - j3)]
                after_zero = False
                for k in range(1, 9):                                # (3.3) counter-clockwise from the pixel after (i2, j2)
                    d = CW[(k2 - k) % 8]
                    if f[i3 + d[0], j3 + d[1]] != 0:
                        i4, j4 = i3 + d[0], j3 + d[1]
                        break
                    if d == (0, 1):
                        after_zero = True
                chain.append((i3 - 1, j3 - 1, k2))
                if after_zero:                                       # (3.4)
                    f[i3, j3] = -nbd
                elif f[i3, j3] == 1:
                    f[i3, j3] = nbd
                if (i4, j4) == (i, j) and (i3, j3) == first:         # (3.5)
                    break
                (i2, j2), (i3, j3) = (i3, j3), (i4, j4)
            out.append(chain)
    return out


def approx_simple(chain, ny):
    """(kept points [(x, y)] from the canonical start on, the canonical start's key) of one chain"""
    n = len(chain)
    if n == 1:
        return [chain[0][:2]], (chain[0][0] * ny + chain[0][1], 0)
    keys = [(x * ny + y, c) for x, y, c in chain]
    s = keys.index(min(keys))
    pts = []
    for t in range(s, s + n):
        (xa, ya, _), (xb, yb, _), (xc, yc, _) = chain[(t - 1) % n], chain[t % n], chain[(t + 1) % n]
        if (xb - xa, yb - ya) != (xc - xb, yc - yb):
            pts.append((xb, yb))
    return pts, keys[s]


def masked(labels, compartment=None, valid_codes=None):
    labels = np.asarray(labels)
    if compartment is None:
        return labels
    return np.where(np.isin(np.asarray(compartment), list(valid_codes)), labels, 0)


def label_rings(labels, compartment=None, valid_codes=None):
    """label -> {"ring": [(x, y)] or None when dropped, "n_pixels", "n_borders", "tie", "chain_len", "n_components_hint"}"""
    img = masked(labels, compartment, valid_codes)
    res = {}
    for lab in np.unique(img):
        if lab == 0:
            continue
        ys, xs = np.nonzero(img == lab)
        x0, y0 = xs.min(), ys.min()
        crop = (img[y0:ys.max() + 1, x0:xs.max() + 1] == lab).T
        ny = crop.shape[1]
        cand = []
        for chain in borders(crop):
            pts, key = approx_simple(chain, ny)
            cand.append((-len(pts), key, pts, chain))
        cand.sort(key=lambda c: c[:2])
        n_best, _, pts, chain = cand[0]
        res[int(lab)] = {"ring": [(x + x0, y + y0) for x, y in pts] if -n_best > 2 else None, "n_pixels": len(xs),
                         "n_borders": len(cand), "tie": sum(c[0] == n_best for c in cand) > 1,
                         "chain": [(x + x0, y + y0) for x, y, _ in chain]}
    return res


def expected(labels, compartment=None, valid_codes=None, scale=(1.0, 1.0), translation=(0.0, 0.0)):
    """what label_contours returns, as numpy arrays, and the counters by name"""
    res = label_rings(labels, compartment, valid_codes)
    kept = [l for l in sorted(res) if res[l]["ring"] is not None]
    rings = [np.asarray(res[l]["ring"], np.float64).reshape(-1, 2) for l in kept]
    offs = np.zeros(len(kept) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in rings])
    xy = np.concatenate(rings) if rings else np.zeros((0, 2))
    xy = xy * np.asarray(scale, np.float64) + np.asarray(translation, np.float64)
    c = {"n_present": len(res), "n_kept": len(kept), "n_vertices": int(offs[-1]), "n_dropped": len(res) - len(kept),
         "n_borders": sum(r["n_borders"] for r in res.values()), "longest_ring": max([len(r) for r in rings], default=0),
         "n_ties": sum(r["tie"] for r in res.values()), "n_bad_label": 0, "overflow": 0}
    return {"ring_offsets": offs, "xy": xy, "label_ids": np.asarray(kept, np.int32),
            "n_pixels": np.asarray([res[l]["n_pixels"] for l in kept], np.int64), "counters": c, "by_label": res}


# ---------------------------------------------------------------- shapes ---
def art(rows):
    """[(x, y)] of the '#' of an ASCII drawing (row = y, column = x)"""
    return [(x, y) for y, row in enumerate(rows) for x, ch in enumerate(row) if ch == "#"]


# name -> (drawing, the ring by hand or None when the label is dropped).  Worked by hand from the contract: start at the
# first pixel of the x-major scan, travel as border following does (down the first column of the transposed crop, i.e.
# towards larger x first along the side that has background at y - 1).
HAND = {
    "L3": (["#.", "##"], [(0, 0), (1, 1), (0, 1)]),
    "block2": (["##", "##"], [(0, 0), (1, 0), (1, 1), (0, 1)]),
    # outer border: the 4 corners; hole border: the 4 edge midpoints, first pixel of the scan (0, 1).  A tie: the outer
    # border starts at (0, 0), which comes first
    "ring3": (["###", "#.#", "###"], [(0, 0), (2, 0), (2, 2), (0, 2)]),
    "line5": (["#####"], None),
    # 8-connected: the chain steps diagonally from arm to arm and never visits the centre
    "plus": ([".#.", "###", ".#."], [(0, 1), (1, 0), (2, 1), (1, 2)]),
    "diag2": (["#.", ".#"], None),
    "diag5": (["#....", ".#...", "..#..", "...#.", "....#"], None),
}
HAND_ORDER = ("L3", "block2", "ring3", "line5", "plus", "diag2", "diag5")


def place(img, pts, label, x0, y0):
    for x, y in pts:
        assert img[y0 + y, x0 + x] == 0
        img[y0 + y, x0 + x] = label


def hand_image():
    """the hand cases as labels 1 .. 7 of one 32 x 48 image (H != W) -> (labels, {label: ring or None})"""
    img = np.zeros((32, 48), np.int32)
    want = {}
    for k, name in enumerate(HAND_ORDER):
        x0, y0 = 2 + 6 * k, 3 + 3 * k
        rows, ring = HAND[name]
        place(img, art(rows), k + 1, x0, y0)
        want[k + 1] = None if ring is None else [(x + x0, y + y0) for x, y in ring]
    return img, want


def comb(n_candidates):
    """a one-border shape with exactly n_candidates pixels that have background at y - 1: teeth on a base line"""
    teeth = (n_candidates + 1) // 2
    pts = [(x, 2) for x in range(2 * teeth - 1)] + [(2 * t, y) for t in range(teeth) for y in (0, 1)]
    if n_candidates % 2 == 0:
        pts += [(2 * teeth - 1, 2)]                                  # one more base pixel: one more candidate
    return pts


def spiral(n):
    """a one-pixel-wide square spiral in an n x n box, arms two apart"""
    x, y, dx, dy = 0, 0, 1, 0
    pts = [(x, y)]
    steps = [n - 1, n - 1, n - 1]
    k = n - 3
    while k > 0:
        steps += [k, k]
        k -= 2
    for s in steps:
        for _ in range(s):
            x, y = x + dx, y + dy
            pts.append((x, y))
        dx, dy = -dy, dx
    return pts


def hole_comb(teeth):
    """a solid rectangle with a comb-shaped hole: the hole border has more kept points than the outer border's 4"""
    w, h = 2 * teeth + 3, 7
    hole = {(x, 4) for x in range(2, w - 2)} | {(2 + 2 * t, y) for t in range(teeth) for y in (2, 3)}
    return [(x, y) for x in range(w) for y in range(h) if (x, y) not in hole]


def edge_cases():
    """name -> labels [H, W] int32"""
    c = {}
    a = np.zeros((9, 13), np.int32)
    a[4, :] = 3
    a[:, 6] = 3
    c["touches_all_four_borders"] = a
    c["fills_the_image"] = np.full((7, 5), 2, np.int32)
    a = np.zeros((6, 10), np.int32)
    a[:, :5], a[:, 5:] = 1, 2
    c["two_adjacent_no_background"] = a
    yy, xx = np.mgrid[0:8, 0:9]
    c["checkerboard"] = np.where((xx + yy) % 2 == 0, 5, 0).astype(np.int32)
    a = np.zeros((12, 16), np.int32)
    place(a, art(["##", "##"]), 1, 1, 1)
    place(a, art(["#...", "#...", "####", "####"]), 1, 8, 5)
    c["two_components"] = a
    a = np.zeros((9, 20), np.int32)
    place(a, hole_comb(6), 4, 2, 1)
    c["hole_outnumbers_outer"] = a
    a = np.zeros((12, 12), np.int32)                                 # > 64 chain steps
    place(a, spiral(10), 1, 1, 1)
    c["spiral_64"] = a
    a = np.zeros((72, 72), np.int32)                                 # > 4096 chain steps
    place(a, spiral(70), 1, 1, 1)
    c["spiral_4096"] = a
    a = np.zeros((10, 24), np.int32)
    for k, lab in enumerate((1, 7, 65537)):
        place(a, art(["##.", "###", ".##"]), lab, 2 + 7 * k, 3)
    c["sparse_ids"] = a
    # the candidate queue of the trace kernel drains at 64: one below, at, one above, and the same around 128
    a = np.zeros((6 * 5, 140), np.int32)
    for k, n in enumerate((63, 64, 65, 127, 128, 129)):
        place(a, comb(n), k + 1, 1, 1 + 5 * k)
    c["candidate_queue_boundaries"] = a
    # the LDS route ends at 32768 padded bits: 128 columns x 256 rows fits, 257 rows do not; 65 columns take a second
    # 64-pixel chunk per row and 33 a second word
    a = np.zeros((260, 400), np.int32)
    a[1:257, 1:129] = 1
    a[1:258, 131:259] = 2
    a[1:30, 262:326] = 3
    a[1:30, 330:395] = 4
    a[40:60, 262:294] = 5
    a[40:60, 300:333] = 6
    a[100:103, 300:303] = 0
    c["lds_route_boundaries"] = a
    # the offsets kernel scans 1024 labels per trip: 1023, 1024, 1025 present labels of 2 x 2 pixels
    for n in (1023, 1024, 1025):
        a = np.zeros((3 * 33, 3 * 32 + 1), np.int32)
        for k in range(n):
            y, x = 3 * (k // 32), 3 * (k % 32)
            a[y:y + 2, x:x + 2] = k + 1
        c[f"labels_{n}"] = a
    return c


def long_ring():
    """one label whose ring has more than SEGGER_MORPH_MAX_VERTS kept points: a comb of 1500 teeth"""
    a = np.zeros((5, 3003), np.int32)
    place(a, comb(2999), 9, 1, 1)
    return a


def voronoi(size, n_seeds, gap, seed):
    """a label image: every pixel takes the nearest seed's label unless that seed is farther than ``gap``"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, size, (n_seeds, 2))
    yy, xx = np.mgrid[0:size, 0:size]
    d2 = (xx[..., None] - pts[:, 0]) ** 2 + (yy[..., None] - pts[:, 1]) ** 2
    lab = d2.argmin(-1) + 1
    return np.where(d2.min(-1) > gap * gap, 0, lab).astype(np.int32)


def voronoi_small():
    return voronoi(96, 40, 7.0, 3)


def voronoi_medium():
    return voronoi(256, 150, 10.0, 5)


# ---------------------------------------------------------------- independent properties ---
def on_segment(px, py, ax, ay, bx, by):
    return (bx - ax) * (py - ay) == (by - ay) * (px - ax) and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by)


def inside_or_on(ring, px, py):
    """exact integer even-odd test of the point against the closed ring, its edges included"""
    n, inside = len(ring), False
    for k in range(n):
        (ax, ay), (bx, by) = ring[k], ring[(k + 1) % n]
        if on_segment(px, py, ax, ay, bx, by):
            return True
        if (ay > py) != (by > py):
            # x of the edge at height py, compared without dividing: px < ax + (py - ay) (bx - ax) / (by - ay)
            lhs, rhs = (px - ax) * (by - ay), (py - ay) * (bx - ax)
            if (lhs < rhs) == (by > ay):
                inside = not inside
    return inside


def raster(ring):
    """(the lattice points inside or on the ring, those strictly inside); outside the ring's bounding box there are none"""
    xs, ys = [p[0] for p in ring], [p[1] for p in ring]
    n = len(ring)
    closed, strict = set(), set()
    for x in range(min(xs), max(xs) + 1):
        for y in range(min(ys), max(ys) + 1):
            if inside_or_on(ring, x, y):
                closed.add((x, y))
                if not any(on_segment(x, y, *ring[k], *ring[(k + 1) % n]) for k in range(n)):
                    strict.add((x, y))
    return closed, strict


def boundary_lattice_points(ring):
    n = len(ring)
    return sum(int(np.gcd(abs(ring[(k + 1) % n][0] - ring[k][0]), abs(ring[(k + 1) % n][1] - ring[k][1]))) for k in range(n))


def shoelace2(ring):
    n = len(ring)
    return abs(sum(ring[k][0] * ring[(k + 1) % n][1] - ring[(k + 1) % n][0] * ring[k][1] for k in range(n)))


def admitted(labels, res):
    """the labels the property checks apply to: one 8-connected component, no hole, a chain that visits no pixel twice"""
    from scipy import ndimage
    ok = []
    for lab, r in res.items():
        if r["ring"] is None:
            continue
        m = labels == lab
        if ndimage.label(m, structure=np.ones((3, 3)))[1] != 1:
            continue
        if ndimage.binary_fill_holes(m).sum() != m.sum():            # 4-connected background: the hole borders' rule
            continue
        if len(set(r["chain"])) != len(r["chain"]):
            continue
        ok.append(lab)
    return ok
