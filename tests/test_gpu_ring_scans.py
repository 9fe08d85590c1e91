"""The one-workgroup scan of csrc/post_common.h (GroupScan) under each of its five users, through the public entry points:
the offsets an entry point returns -- or, where it returns none, the list those offsets place -- against a numpy cumulative
sum of per-item counts that follow from how the input is built, never from the code under test.  Item counts 1, 64, 65, W,
W + 1 and 2 W + 1 with W the scan's workgroup width: the wave edge, the chunk edge, and a carry over two chunk boundaries.
The counts vary from item to item (and some items are dropped), so a sum that loses or doubles a wave's total shows."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "segger_amd", "csrc")


def constant(file, name):
    m = re.search(r"\b%s = (\d+)\b" % name, open(os.path.join(CSRC, file)).read())
    assert m, (file, name)
    return int(m.group(1))


def counts_of(width):
    return (1, 64, 65, width, width + 1, 2 * width + 1)


W = constant("post_common.h", "kScanThreads")                        # counts_to_offsets_kernel
W_SIMPLIFY = constant("simplify.hip", "kSrScanThreads")
W_CELLS = constant("cell_rings.h", "kBndScanThreads")
W_CONTOURS = constant("contours.hip", "kCtOffThreads")


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def ngon(k, cx):
    """a regular k-gon of radius 0.4 around (cx, 0): no three vertices collinear"""
    a = 2.0 * np.pi * np.arange(k) / k
    return np.stack([cx + 0.4 * np.cos(a), 0.4 * np.sin(a)], 1)


def squares(n):
    """n unit squares, two units apart: the CSR"""
    corner = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    xy = (corner[None] + np.stack([2.0 * np.arange(n), np.zeros(n)], 1)[:, None]).reshape(-1, 2)
    return 4 * np.arange(n + 1, dtype=np.int64), xy


def test_the_widths_are_the_documented_ones():
    assert W == W_SIMPLIFY == W_CELLS == 1024 and W_CONTOURS % 64 == 0


@pytest.mark.parametrize("n", counts_of(W_SIMPLIFY))
def test_simplify_rings_offsets(n):
    """sr_scan_kernel: ring i is a 3-, 4- or 5-gon; tolerance 0 keeps every vertex"""
    from segger_amd import simplify_rings
    k = 3 + np.arange(n) % 3
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    xy = np.concatenate([ngon(int(k[i]), float(i)) for i in range(n)])
    out = simplify_rings(t(off), t(xy), 0.0)
    assert np.array_equal(out["ring_offsets"].cpu().numpy(), off)
    assert np.array_equal(out["vertex_index"].cpu().numpy(), np.arange(off[-1]))


@pytest.mark.parametrize("n", counts_of(W))
def test_points_in_polygons_offsets(n):
    """counts_to_offsets_kernel<int64> over the polygons: square i holds 1 + i % 3 points; a list placed by wrong offsets
    would miss a pair or hold a foreign one"""
    from segger_amd import points_in_polygons
    off, xy = squares(n)
    per = 1 + np.arange(n) % 3
    poly = np.repeat(np.arange(n), per)
    rank = np.arange(per.sum()) - np.repeat(np.cumsum(per) - per, per)
    pts = np.stack([2.0 * poly + 0.25 * (1 + rank), np.full(len(poly), 0.5)], 1)
    got = points_in_polygons(t(pts), t(off), t(xy)).cpu().numpy()
    assert np.array_equal(got, np.stack([np.arange(len(poly)), poly]))


@pytest.mark.parametrize("m", counts_of(W))
def test_polygon_overlaps_offsets(m):
    """counts_to_offsets_kernel<int32> over the grid's cells and <int64> over the m = Pa + Pb items of the candidate pass:
    set A is the first ceil(m / 2) unit squares, set B the first floor(m / 2); square i meets square i and no other"""
    from segger_amd import polygon_overlaps
    na, nb = (m + 1) // 2, m // 2
    off_a, xy_a = squares(na)
    off_b, xy_b = squares(nb)
    out = polygon_overlaps(t(off_a), t(xy_a), t(off_b), t(xy_b.reshape(-1, 2)))
    assert np.array_equal(out["pairs"].cpu().numpy(), np.stack([np.arange(nb), np.arange(nb)]))
    assert np.array_equal(out["area"].cpu().numpy(), np.ones(nb))


@pytest.mark.parametrize("n", counts_of(W_CELLS))
@pytest.mark.parametrize("entry", ("cell_boundaries", "cell_outlines"))
def test_cell_ring_offsets(entry, n):
    """bnd_scan_kernel, vertices and kept cells scanned together: cell i is a triangle, a square or (no ring) two points"""
    import segger_amd
    kind = (np.arange(n) + 1) % 3                                    # 1: triangle, 2: square, 0: two points
    shapes = {0: [[0, 0], [1, 1]], 1: [[0, 0], [1, 0], [0, 1]], 2: [[0, 0], [1, 0], [1, 1], [0, 1]]}
    rows = [np.array(shapes[int(kd)], np.float64) + [3.0 * i, 0.0] for i, kd in enumerate(kind)]
    xy = np.concatenate(rows)
    cell = np.repeat(np.arange(n), [len(r) for r in rows]).astype(np.int32)
    out = getattr(segger_amd, entry)(t(xy), t(cell), n)
    kept = np.flatnonzero(kind > 0)
    verts = np.where(kind == 1, 3, 4)[kept]
    assert np.array_equal(out["cell_ids"].cpu().numpy(), kept)
    assert np.array_equal(out["ring_offsets"].cpu().numpy(), np.concatenate([[0], np.cumsum(verts)]))
    assert np.array_equal(out["n_transcripts"].cpu().numpy(), verts)
    assert out["n_dropped"] == n - len(kept)


@pytest.mark.parametrize("n", counts_of(W_CONTOURS))
def test_label_contours_offsets(n):
    """ct_offsets_kernel: label i + 1 is a 2 x 2 block of a strip (4 vertices) or, every third, a 1 x 2 one (2 points: dropped)"""
    from segger_amd import label_contours
    narrow = np.arange(n) % 3 == 2
    labels = np.zeros((2, 2 * n), np.int32)
    labels[:, 0::2] = np.arange(1, n + 1)
    labels[:, 1::2] = np.where(narrow, 0, np.arange(1, n + 1))
    out = label_contours(t(labels))
    kept = np.flatnonzero(~narrow)
    assert np.array_equal(out["label_ids"].cpu().numpy(), kept + 1)
    assert np.array_equal(out["ring_offsets"].cpu().numpy(), 4 * np.arange(len(kept) + 1))
    assert np.array_equal(out["n_pixels"].cpu().numpy(), np.full(len(kept), 4))
