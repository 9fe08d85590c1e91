"""The CPU oracle of the buffered-boundary counts (tests/buffered_count_cases.py) against cases worked by hand, its pair
set against the exact rational predicate on grid coordinates, and its restatement of ``filter_boundaries`` on rings that
straddle each side and each corner of a region.  No GPU, no product import."""
import numpy as np
import pytest

import buffered_count_cases as bc
import polygon_join_cases as pc

SQ = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
#            inside       outside     on an edge  on a vertex  0.125 out     exactly 0.25 out
PTS = np.array([[0.5, 0.5], [2.0, 2.0], [0.5, 0.0], [0.0, 0.0], [1.125, 0.5], [1.25, 0.5]])
GENE = np.array([2, 0, 1, 2, 1, 0])


def row(csr, p):
    a, b = csr["indptr"][p], csr["indptr"][p + 1]
    return dict(zip(csr["indices"][a:b].tolist(), csr["counts"][a:b].tolist()))


@pytest.mark.parametrize("pred,d,want", [
    ("contains", 0.0, {2: 1}),                                       # the open set: the inside point only
    ("intersects", 0.0, {1: 1, 2: 2}),                               # the closed set: + the edge (gene 1) and the vertex (gene 2)
    ("contains", 0.25, {1: 2, 2: 2}),                                # + the point 0.125 out; dist2 == d*d is NOT < d*d
    ("intersects", 0.25, {0: 1, 1: 2, 2: 2}),                        # + the point exactly 0.25 out (gene 0)
])
def test_unit_square_by_hand(pred, d, want):
    got = bc.buffered_counts(PTS, GENE, [SQ], 3, d, pred)
    assert row(got, 0) == want
    assert got["indices"].dtype == np.int32 and np.all(np.diff(got["indices"]) > 0)
    assert got["cell_count"].tolist() == [sum(want.values())]
    assert got["counters"].tolist() == [sum(want.values()), len(want), 0, 0, 0]


def test_a_point_in_two_overlapping_squares_is_counted_twice_and_a_bad_gene_only_in_n_bad():
    rings = [SQ * 2.0, SQ * 2.0 + 1.0]                               # [0, 2]^2 and [1, 3]^2
    pts = np.array([[1.5, 1.5], [0.5, 0.5], [2.5, 2.5], [1.25, 1.75], [9.0, 9.0]])
    gene = np.array([4, 4, 0, 7, 1])                                 # 7 is outside [0, 5)
    got = bc.buffered_counts(pts, gene, rings, 5, 0.0)
    assert row(got, 0) == {4: 2} and row(got, 1) == {0: 1, 4: 1}
    assert got["indptr"].tolist() == [0, 1, 3] and got["cell_count"].tolist() == [2, 2]
    assert got["counters"].tolist() == [6, 3, 2, 0, 0]               # the bad point matches both squares: two bad pairs
    assert bc.dense(got, 5).sum() == got["counters"][0] - got["counters"][2]
    assert np.array_equal(bc.dense(bc.from_dense(bc.dense(got, 5)), 5), bc.dense(got, 5))


def test_overflow_and_large_tier_counters_follow_their_constants():
    rings, pts, gene, n_genes = bc.scene_overflow(40)
    got = bc.buffered_counts(pts, gene, rings, n_genes, 0.0, touched=39, small_genes=39)
    assert np.diff(got["indptr"]).tolist() == [40, 1, 0] and got["counts"][40] == 20
    assert got["counters"].tolist() == [60, 41, 0, 1, 3]
    assert bc.buffered_counts(pts, gene, rings, n_genes, 0.0, touched=40, small_genes=40)["counters"].tolist() == [60, 41, 0, 0, 0]


def test_filter_boundaries_on_every_side_and_corner():
    inset, outset = (0.0, 0.0, 10.0, 10.0), (-2.0, -2.0, 12.0, 12.0)

    def sq(x, y):
        return np.array([[x, y], [x + 2.0, y], [x + 2.0, y + 2.0], [x, y + 2.0]])
    rings = {"inside": sq(4, 4), "left side": sq(-1, 4), "right side": sq(9, 4), "low-y side (the reference's top)": sq(4, -1),
             "high-y side (its bottom)": sq(4, 9), "low-x low-y corner": sq(-1, -1), "low-x high-y corner": sq(-1, 9),
             "high-x low-y corner": sq(9, -1), "high-x high-y corner": sq(9, 9), "in the margin": np.array([[-1.5, 4.0], [-0.5, 4.0], [-0.5, 6.0], [-1.5, 6.0]]),
             "touching the inset's edge from inside": sq(0, 8), "no vertices": np.zeros((0, 2))}
    want = {"inside": True, "left side": True, "right side": False, "low-y side (the reference's top)": True,
            "high-y side (its bottom)": False, "low-x low-y corner": True, "low-x high-y corner": False,
            "high-x low-y corner": False, "high-x high-y corner": False, "in the margin": False,
            "touching the inset's edge from inside": True, "no vertices": True}
    got = bc.filter_boundaries(list(rings.values()), inset, outset)
    assert dict(zip(rings, got.tolist())) == want
    # the four regions that meet in a corner: a ring on the corner, on a shared side, is kept by exactly one of them
    quads = [(-10.0, -10.0, 0.0, 0.0), (0.0, -10.0, 10.0, 0.0), (-10.0, 0.0, 0.0, 10.0), (0.0, 0.0, 10.0, 10.0)]
    for ring in (sq(-1, -1), sq(-1, 4), sq(4, -1), sq(3, 3)):
        keeps = [bool(bc.filter_boundaries([ring], q, (q[0] - 2, q[1] - 2, q[2] + 2, q[3] + 2))[0]) for q in quads]
        assert sum(keeps) == 1, (ring.tolist(), keeps)


@pytest.mark.parametrize("d", pc.D_CASES)
@pytest.mark.parametrize("pred", pc.PREDICATES)
def test_pair_set_equals_the_exact_rational_predicate(pred, d):
    rings, _, points, labels, _ = pc.cases()
    ref = pc.reference("cases", d)
    got = bc.pairs(points, rings, np.full(len(rings), d), pred)
    g = {tuple(r) for r in pc.without(got, ref["undecided"]).tolist()}
    w = {tuple(r) for r in pc.without(ref["exact"][pred], ref["undecided"]).tolist()}
    assert g == w and len(w) > 100
    assert len(ref["undecided"]) <= pc.MAX_UNDECIDED * len(w)


def test_region_sum_equals_one_call_when_every_polygon_is_kept_once():
    rings, points = bc.scene_field()
    gene = bc.field_genes(60)
    one = bc.buffered_counts(points, gene, rings, 60, 1.5)
    reg = bc.buffered_counts_regions(points, gene, rings, 60, bc.REGION_GRID, 1.5, bc.REGION_OVERLAP)
    assert reg["kept"].min() >= 1 and reg["kept"].max() == 1
    for k in ("indptr", "indices", "counts", "cell_count"):
        assert np.array_equal(reg[k], one[k]), k
