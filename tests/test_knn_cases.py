"""The inputs of the grid kNN tests decide what they are meant to decide (CPU): tests/knn_cases.py has the conditions.
Also: the cases contain what their names say, the checker accepts the reference and refuses the answers of the walk
that trusts exact cell coordinates and of the inclusive bound (tests/knn_cases.py::emulate_walk, the kernel's float32
operations in numpy), and the grid rule keeps its promises."""
import math

import numpy as np
import pytest

import knn_cases as kc
from segger_amd.neighbors import grid_rule

F = np.float32


@pytest.fixture(scope="module")
def cases():
    return kc.all_cases()


def emulated(case, sound, strict):
    """The emulated walk over every query -> (nbr int32, dist float32) as the kernel would write them."""
    m = len(case["points"] if case["queries"] is None else case["queries"])
    rows = [kc.emulate_walk(case, i, sound=sound, strict=strict) for i in range(m)]
    nbr = np.array([r[1] for r in rows], dtype=np.int32)
    dist = np.sqrt(np.array([r[0] for r in rows], dtype=F))
    return nbr, (dist if case.get("dist", True) else None)


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_is_certified(cases, name):
    assert (kc.RTOL, kc.MARGIN) == (1e-6, 1e-5)
    assert kc.certify(cases[name]) >= kc.MARGIN


def test_scipy_bound_is_strict():
    """The reference the cases are built against: scipy's distance_upper_bound excludes the point at exactly the bound."""
    from scipy.spatial import cKDTree
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    d, i = cKDTree(pts).query(pts[:1], k=3, distance_upper_bound=1.0)
    assert d.tolist() == [[0.0, math.inf, math.inf]] and i.tolist() == [[0, 3, 3]]
    ref_d, ref_i = kc.reference(kc.case(pts, pts[:1], k=3, max_dist=1.0))
    assert np.array_equal(ref_d, d) and np.array_equal(ref_i, i)


@pytest.mark.parametrize("name", ["lattice_strict_d5_k64", "k_caps_n300_k17", "degenerate_duplicates_x4_self",
                                  "degenerate_negative_query", "abi_grids_middle_third_self_bounded", "stop_python_grid"])
def test_reference_is_the_kdtree(cases, name):
    from scipy.spatial import cKDTree
    case = cases[name]
    pts = case["points"].astype(np.float64)
    qs = pts if case["queries"] is None else case["queries"].astype(np.float64)
    d, _ = cKDTree(pts).query(qs, k=case["k"], distance_upper_bound=case["max_dist"])
    ref_d, ref_i = kc.reference_of(name)
    assert np.array_equal(np.isinf(d.reshape(ref_d.shape)), ref_i == len(pts))
    assert np.allclose(d.reshape(ref_d.shape), ref_d, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", [n for n in kc.NAMES if n.startswith(("stop_", "lattice_"))])
def test_checker_tells_the_walks_apart(cases, name):
    """The checker accepts the reference's own answer and the float32-sound, strict walk, and refuses the walk it was
    built against: the evidence (short of a GPU) that the GPU test fails on a kernel with that walk."""
    case = cases[name]
    if name == "stop_python_grid":                                       # 4000 rows: the adversarial ones and a sample
        rows = sorted({a["query"] for a in case["adversarial"]} | set(range(0, 4000, 97)))
        case = dict(case, queries=case["points"][rows])
        ref_d, ref_i = kc.reference(case)
    else:
        ref_d, ref_i = kc.reference_of(name)
    want_dist = case.get("dist", True)
    kc.check(case, ref_i.astype(np.int32), ref_d.astype(F) if want_dist else None, ref_d)
    kc.check(case, *emulated(case, sound=True, strict=True), ref_d)
    old = emulated(case, sound=False, strict=False) if name.startswith("lattice_") else emulated(case, sound=False, strict=True)
    with pytest.raises(AssertionError, match="padding differs|off the reference"):
        kc.check(case, *old, ref_d)


def test_checker_refuses_wrong_answers(cases):
    case = cases["k_caps_n300_k9"]
    ref_d, ref_i = kc.reference_of("k_caps_n300_k9")
    nbr, dist = ref_i.astype(np.int32), ref_d.astype(F)
    kc.check(case, nbr, dist, ref_d)
    bad = nbr.copy()
    bad[5, 3] = bad[5, 2]                                                # an id twice (its distance is off as well)
    with pytest.raises(AssertionError):
        kc.check(case, bad, dist, ref_d)
    bad = nbr.copy()
    bad[7, [1, 2]] = bad[7, [2, 1]]                                      # ids in the wrong order: they no longer match dist
    with pytest.raises(AssertionError, match="id beside it|off the reference"):
        kc.check(case, bad, dist, ref_d)
    bad = dist.copy()
    bad[11, 4] *= F(1 + 3e-6)
    with pytest.raises(AssertionError, match="dist is"):
        kc.check(case, nbr, bad, ref_d)
    bad = nbr.copy()
    bad[0, 8] = len(case["points"])
    with pytest.raises(AssertionError, match="padding differs"):
        kc.check(case, bad, dist, ref_d)
    short = cases["k_caps_n20_k33"]
    ref_d, ref_i = kc.reference_of("k_caps_n20_k33")
    dist = ref_d.astype(F)
    dist[3, 30] = F(0)
    with pytest.raises(AssertionError, match=r"\+inf"):
        kc.check(short, ref_i.astype(np.int32), dist, ref_d)
    dup = cases["degenerate_duplicates_x4_self"]                         # ties: any of the four copies is right, once
    ref_d, ref_i = kc.reference_of("degenerate_duplicates_x4_self")
    nbr = ref_i.astype(np.int32)
    nbr[:, :4] = nbr[:, [3, 1, 0, 2]]
    kc.check(dup, nbr, ref_d.astype(F), ref_d)
    nbr[:, 1] = nbr[:, 0]
    with pytest.raises(AssertionError, match="twice"):
        kc.check(dup, nbr, ref_d.astype(F), ref_d)


def test_cases_hold_what_they_claim(cases):
    assert list(cases) == kc.NAMES and len(set(kc.NAMES)) == len(kc.NAMES)
    for name, case in cases.items():
        n = len(case["points"])
        assert n <= 5000 and (case["grid"] == "python" or len(case["grid"]) == 5), name
    # lattice: 12 x 12 integers, self query, and a neighbour at exactly max_dist for every bound
    for max_dist, k in kc.LATTICE:
        for suffix in ("", "_abi"):
            case = cases[f"lattice_strict_d{int(max_dist)}_k{k}{suffix}"]
            assert len(case["points"]) == 144 and case["queries"] is None and case["max_dist"] == max_dist
            d = np.hypot(*(case["points"][:, None, :] - case["points"][None, :, :]).transpose(2, 0, 1).astype(np.float64))
            assert (d == max_dist).sum() >= 144 * 2
            assert (case["grid"] == "python") == (suffix == "") and (suffix == "" or case["grid"][2] != max_dist)
    on_345 = cases["lattice_strict_d5_k64"]["points"]
    assert ((on_345 == (3, 4)).all(1)).any() and ((on_345 == (4, 3)).all(1)).any()
    # stop_maxdist: cell == max_dist on an explicit grid, r = 1, both directions, in x and in y
    for name, axis in (("stop_maxdist_x", 0), ("stop_maxdist_x_wide_cell", 0), ("stop_maxdist_y", 1)):
        case = cases[name]
        assert case["grid"][2] == case["max_dist"] and len(case["adversarial"]) >= 6
        signs = {float(np.sign(case["points"][a["p"]][axis] - case["queries"][a["query"]][axis])) for a in case["adversarial"]}
        assert signs == {1.0, -1.0} and all(a["r"] == 1 and a["a"] is None for a in case["adversarial"])
        other = 1 - axis
        assert all(case["points"][a["p"]][other] == case["queries"][a["query"]][other] for a in case["adversarial"])
    # stop_kth: no bound, k = 1 and 3, r = 1 and 2, A in ring <= r and farther than P
    for k in (1, 3):
        for r in (1, 2):
            case = cases[f"stop_kth_k{k}_r{r}"]
            assert case["k"] == k and math.isinf(case["max_dist"]) and len(case["adversarial"]) >= 4
            grid = case["grid"]
            for a in case["adversarial"]:
                ring_a = np.abs(kc.cells_of(case["points"][a["a"]][None], grid) - kc.cells_of(case["queries"][a["query"]][None], grid))
                assert a["r"] == r and ring_a.max() <= r
    assert cases["stop_kth_k3_r1_y"]["grid"][3] < cases["stop_kth_k3_r1_y"]["grid"][4]
    # stop_python_grid: the real grid rule picks cell == max_dist, tens of thousands of columns, one row
    case = cases["stop_python_grid"]
    x0, y0, cell, nx, ny = kc.python_grid(case)
    assert case["grid"] == "python" and cell == case["max_dist"] and 10_000 <= nx <= 30_001 and ny == 1
    assert len(case["adversarial"]) >= 6 and case["queries"] is None
    # k_caps: both sides of every capacity, and n < k
    assert kc.K_CAPS == (8, 9, 16, 17, 32, 33, 64)
    assert all(len(cases[f"k_caps_n300_k{k}"]["points"]) == 300 and len(cases[f"k_caps_n20_k{k}"]["points"]) == 20 for k in kc.K_CAPS)
    assert np.isinf(kc.reference_of("k_caps_n20_k33")[0]).sum() == 20 * 13
    # degenerate
    for name in ("coincident", "coincident_far"):
        pts = cases[f"degenerate_{name}_self"]["points"]
        assert len(pts) == 500 and (pts == pts[0]).all()
        assert (kc.reference_of(f"degenerate_{name}_self")[0] == 0).all()
    assert cases["degenerate_coincident_far_self"]["points"][0].tolist() == [8191.5, 16383.25]
    clumps = cases["degenerate_two_clumps_self"]["points"]
    assert len(np.unique(clumps, axis=0)) == 2 and kc.reference_of("degenerate_two_clumps_self")[0].max() == 1000.0
    assert np.unique(cases["degenerate_horizontal_line_self"]["points"][:, 1]).size == 1
    assert np.unique(cases["degenerate_vertical_line_self"]["points"][:, 0]).size == 1
    assert kc.python_grid(cases["degenerate_horizontal_line_self"])[3:] == (30001, 1)
    assert len(cases["degenerate_n1_k5_self"]["points"]) == 1 and cases["degenerate_n1_k5_self"]["k"] == 5
    assert len(cases["degenerate_n2_query"]["points"]) == 2
    dup = cases["degenerate_duplicates_x4_self"]
    assert dup["k"] == 6 and len(dup["points"]) == 1000 and len(np.unique(dup["points"], axis=0)) == 250
    assert (kc.reference_of("degenerate_duplicates_x4_self")[0][:, :4] == 0).all()
    crowd = cases["degenerate_outlier_one_cell_self"]
    cells = kc.cells_of(crowd["points"], kc.python_grid(crowd))
    assert len(crowd["points"]) == 2000 and (cells[:-1] == cells[0]).all() and (cells[-1] != cells[0]).all()
    assert cases["degenerate_negative_self"]["points"].max() < 0
    for name in kc.NAMES:
        if name.startswith("degenerate_"):
            assert (cases[name]["queries"] is None) == name.endswith("_self"), name
    # abi_grids: the same points and queries under every grid; NULL queries and NULL dist are covered
    base = cases["abi_grids_one_cell"]
    pts, qs = base["points"], base["queries"]
    assert len(pts) == 400 and len(qs) == 100 and base["grid"][3:] == (1, 1)
    for name in (n for n in kc.NAMES if n.startswith("abi_grids_")):
        case = cases[name]
        assert case["points"] is pts or np.array_equal(case["points"], pts)
        assert (case["queries"] is None) == name.endswith("_self_bounded") and case.get("dist", True) == (not name.endswith("_no_dist"))
        assert case["queries"] is None or np.array_equal(case["queries"], qs)
        assert max(case["grid"][3:]) <= 512
    both = np.concatenate([pts, qs])
    x0, y0, cell, nx, ny = cases["abi_grids_middle_third"]["grid"]
    inside = (both[:, 0] >= x0) & (both[:, 0] < x0 + nx * cell) & (both[:, 1] >= y0) & (both[:, 1] < y0 + ny * cell)
    assert 0.02 < inside.mean() < 0.5                                    # most points and queries clamp into edge cells
    x0, y0, cell, nx, ny = cases["abi_grids_off_grid"]["grid"]
    assert (qs[:, 0] < x0).all() and (pts[:, 0] < x0).all()
    assert cases["abi_grids_coarse"]["grid"][2] >= 10 * math.sqrt(2 * 100 * 100 / 400) * 0.99


def test_grid_rule():
    """What knn_grid promises of its grid, over the cases' boxes and a sweep: <= 4n cells up to the rounding of nx and ny
    (4n + nx + ny; 4n + O(sqrt n) for a box that is no strip), <= 30001 along an axis, cell <= max_dist unless a cap binds."""
    rng = np.random.default_rng(0)
    boxes = [(0.0, 0.0, w, h, n, md) for w in (0.0, 1e-3, 1.0, 50.0, 1e4, 1e6) for h in (0.0, 0.3, 50.0, 1e6)
             for n in (1, 2, 300, 5000, 1_000_000) for md in (math.inf, 0.5, 3.0)]
    boxes += [(float(a), float(b), float(a + w), float(b + h), int(n), math.inf)
              for a, b, w, h, n in zip(rng.uniform(-1e4, 1e4, 200), rng.uniform(-1e4, 1e4, 200), rng.uniform(0, 2e4, 200),
                                       rng.uniform(0, 2e4, 200), rng.integers(1, 10 ** 6, 200))]
    for x0, y0, x1, y1, n, md in boxes:
        cell, nx, ny = grid_rule(x0, y0, x1, y1, n, md)
        assert cell > 0 and nx >= 1 and ny >= 1 and max(nx, ny) <= 30001, (x0, y0, x1, y1, n, md)
        assert nx * ny <= 4 * n + nx + ny and nx * ny < 2 ** 31
        if max(nx, ny) <= 4 * min(nx, ny):
            assert nx * ny <= 4 * n + 10 * math.sqrt(n) + 4
        w, h = max(x1 - x0, 1e-6), max(y1 - y0, 1e-6)
        assert x0 + nx * cell >= x1 and y0 + ny * cell >= y1                 # the grid covers the box
        if math.isfinite(md) and cell > md:
            assert cell in (math.sqrt(w * h / (4.0 * n)), max(w, h) / 30000.0)
    assert grid_rule(0.0, 0.0, 1000.0, 1000.0, 1_000_000) == (math.sqrt(2.0), 708, 708)
    assert grid_rule(0.0, 0.0, 11.0, 11.0, 144, 1.0) == (1.0, 12, 12)
