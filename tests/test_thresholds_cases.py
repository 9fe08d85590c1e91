"""The inputs of the per-gene threshold tests are well-conditioned for the float64 oracle (CPU): tests/thresholds_cases.py
has the conditions.  Also: the cases contain what they are meant to contain."""
import numpy as np
import pytest

import thresholds_cases as tc


@pytest.fixture(scope="module")
def cases():
    return tc.all_cases()


@pytest.mark.parametrize("name", ["slide0", "slide1", "slide2", "slide7_max_iter6", "sizes", "edges", "large", "known"])
def test_case_is_certified(cases, name):
    assert tc.certify(cases[name]) > tc.MARGIN


def test_cases_hold_what_they_claim(cases):
    assert set(cases) == {"slide0", "slide1", "slide2", "slide7_max_iter6", "sizes", "edges", "large", "known"}
    ref = tc.reference(cases["sizes"])
    assert ref["count"].tolist() == list(tc.SIZES) and tc.CHUNK == 1024
    assert (cases["sizes"]["cell"] < 0).sum() == 300
    few = tc.reference(cases["slide7_max_iter6"])
    assert 0 < few["failed_genes"].size < 9                            # some genes fail, some vote for the median
    assert np.allclose(few["threshold"][few["failed_genes"]], few["global_threshold"])
    edges = cases["edges"]
    ref = tc.reference(edges)
    assert np.flatnonzero(ref["count"] == 0).tolist() == [1, 4, 7, 8, 11, 12, 13, 14] and np.isnan(ref["threshold"][[1, 14]]).all()
    zeros = tc.gene_values(edges, 5)
    assert np.signbit(zeros[zeros == 0]).any() and not np.signbit(zeros[zeros == 0]).all()
    assert np.array_equal(np.unique(tc.gene_values(edges, 9)) * 64, np.arange(65))
    assert tc.reference(cases["large"])["count"].tolist() == [50, tc.LARGE, 700, 0, 3]
    known = tc.reference(cases["known"])
    assert abs(known["li"][0] - 0.5) < 1e-12 and abs(known["threshold"][0] - (0.25 + 0.5 / 512)) < 1e-12
    assert known["li"][1] == float(np.float32(0.4))
