"""The index-parity proof can fail, and the designed inputs of the head's route test are what they claim (CPU):
tests/index_parity.py has the rules.  Planted cases on oracle outputs alone: the helper accepts exactly the legitimate
ones; every designed input carries the float64 gap certificate and holds the rows its test asserts."""
import numpy as np
import pytest
import torch

import index_parity as ip

TOL = 2e-6


@pytest.fixture(scope="module")
def scored(oracle):
    """Oracle outputs of a small problem: rows 0..2 without an edge, every other row with several candidates."""
    g = torch.Generator().manual_seed(5)
    n_tx, n_bd, E = 60, 12, 400
    z_tx, z_bd = torch.randn(n_tx, 16, generator=g, dtype=torch.float64), torch.randn(n_bd, 16, generator=g, dtype=torch.float64)
    src, dst = torch.randint(3, n_tx, (E,), generator=g), torch.randint(0, n_bd, (E,), generator=g)
    bd_index = torch.randperm(n_bd, generator=g) + 100
    ei = torch.stack([src, dst])
    score = oracle.edge_scores(z_tx, z_bd, ei).numpy()
    top = np.full(n_tx, -np.inf)
    np.maximum.at(top, src.numpy(), score)
    runner = {}                                                # row -> edge id of its best candidate of ANOTHER boundary
    for r in range(3, n_tx):
        e = np.flatnonzero(src.numpy() == r)
        best_dst = dst.numpy()[e[score[e].argmax()]]
        other = e[dst.numpy()[e] != best_dst]
        if other.size:
            runner[r] = int(other[score[other].argmax()])
    assert len(runner) > 40
    return {"z": (z_tx, z_bd), "ei": ei, "src": src.numpy(), "dst": dst.numpy(), "bd_index": bd_index, "score": score, "top": top,
            "runner": runner, "n": n_tx, "E": E}


def proof(s, seg, score=None, **kw):
    return ip.explain_mismatches(seg, s["src"], s["dst"], s["score"] if score is None else score, s["n"], dst_index=s["bd_index"],
                                 tol=kw.pop("tol", TOL), **kw)


def assigned(oracle, s, min_similarity=None):
    return oracle.predict_assign(*s["z"], s["ei"], s["bd_index"], min_similarity)[0].numpy().copy()


def test_reference_assignment_is_the_oracles(oracle, scored):
    for min_sim in (None, 0.2, float(scored["top"][7])):                 # (a threshold exactly on a row's maximum: >=)
        seg, max_sim = oracle.predict_assign(*scored["z"], scored["ei"], scored["bd_index"], min_sim)
        got, top, arg = ip.reference_assign(scored["src"], scored["dst"], scored["score"], scored["n"], scored["bd_index"], min_sim)
        assert np.array_equal(got, seg.numpy()) and (min_sim is None or (got == -1).sum() > 3)
        assert np.array_equal(arg, oracle.scatter_max(torch.from_numpy(scored["score"]), scored["ei"][0], scored["n"])[1].numpy())
        assert np.array_equal(np.where(np.isinf(top), 0.0, top), max_sim.numpy())
    assert got[7] != -1


def test_proof_accepts_the_legitimate_cases(oracle, scored):
    seg = assigned(oracle, scored)
    empty_eid, empty_sim = np.full(scored["n"], scored["E"]), np.zeros(scored["n"])
    assert proof(scored, seg, max_eid=empty_eid, max_sim=empty_sim) == (0, 0.0)
    assert proof(scored, assigned(oracle, scored, 0.2), min_similarity=0.2) == (0, 0.0)
    # two candidates 1e-9 apart in the reference, the other one taken
    r, e = next(iter(scored["runner"].items()))
    score = scored["score"].copy()
    score[e] = scored["top"][r] - 1e-9
    seg[r] = scored["bd_index"][scored["dst"][e]]
    n, gap = proof(scored, seg, score)
    assert n == 1 and 0.5e-9 < gap < 2e-9
    # ... and as far apart as two scores each off by tol can be
    score[e] = scored["top"][r] - 1.9 * TOL
    assert proof(scored, seg, score)[0] == 1
    # a threshold within tol of a row's maximum: either side may assign
    seg = assigned(oracle, scored)
    for sign in (+1, -1):
        min_sim = float(scored["top"][r]) + sign * TOL / 2
        flipped = assigned(oracle, scored, min_sim)
        assert (flipped[r] == -1) == (sign > 0)
        flipped[r] = seg[r] if sign > 0 else -1
        assert proof(scored, flipped, min_similarity=min_sim) == (1, 0.0)


def test_proof_raises_on_everything_else(oracle, scored):
    seg = assigned(oracle, scored)
    r, e = next(iter(scored["runner"].items()))
    taken = int(scored["bd_index"][scored["dst"][e]])

    def refused(what, seg_bad, score=None, **kw):
        with pytest.raises(AssertionError, match=what):
            proof(scored, seg_bad, score, **kw)

    def with_row(value, row=r, base=seg):
        out = base.copy()
        out[row] = value
        return out
    # a swap across ten tolerances
    score = scored["score"].copy()
    score[e] = scored["top"][r] - 10 * TOL
    refused("swap across more than 2 tol", with_row(taken), score)
    refused("swap across more than 2 tol", with_row(taken), scored["score"])        # ... and across the real gap
    # a boundary that is nobody's candidate, and one that is only another row's
    refused("non-candidate", with_row(7))
    elsewhere = next(int(b) for b in scored["bd_index"] if int(b) not in scored["bd_index"][scored["dst"][scored["src"] == r]].tolist())
    refused("non-candidate", with_row(elsewhere))
    # an empty row that was assigned, or carries the wrong max_eid / max_sim
    refused("empty row is not -1", with_row(taken, row=1))
    refused("max_eid is not E", seg, max_eid=np.zeros(scored["n"], dtype=np.int64))
    refused("max_sim is not 0", seg, max_sim=np.full(scored["n"], 1e-30))
    # -1 where the reference assigns, and no threshold to blame
    refused("without a similarity threshold", with_row(-1))
    # a threshold flip ten tolerances from the threshold, both ways round
    for sign in (+1, -1):
        min_sim = float(scored["top"][r]) + sign * 10 * TOL
        base = assigned(oracle, scored, min_sim)
        refused("farther than tol from the threshold", with_row(seg[r] if sign > 0 else -1, base=base), min_similarity=min_sim)
    # what the proof is for: a head that never looks at a row's first slot, its last slot, or takes the last of equal scores
    first = np.full(scored["n"], scored["E"])
    np.minimum.at(first, scored["src"], np.arange(scored["E"]))
    last = np.full(scored["n"], -1)
    np.maximum.at(last, scored["src"], np.arange(scored["E"]))
    for dropped in (first, last):
        keep = np.ones(scored["E"], dtype=bool)
        keep[dropped[(dropped >= 0) & (dropped < scored["E"])]] = False
        blind, _, _ = ip.reference_assign(scored["src"][keep], scored["dst"][keep], scored["score"][keep], scored["n"], scored["bd_index"])
        assert 0 < (blind != seg).mean() < 0.5
        refused("swap across more than 2 tol|without a similarity threshold", blind)


# ------------------------------------------------------------------------------------------------ designed inputs
SHAPES = sorted({(c, n) for _, c, n in ip.routes()})


@pytest.mark.parametrize("dtype", ip.DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("channels,n_rows", SHAPES)
def test_designed_case_is_certified(dtype, channels, n_rows):
    case = ip.designed_case(channels, n_rows, dtype)
    assert ip.certify(case) >= ip.MIN_GAP
    # ... and holds what it claims: the degree cycle, the last row not empty, edge ids that differ from slots, the winner's slot
    deg = np.bincount(case["src"].numpy(), minlength=n_rows)
    assert deg.tolist() == case["degrees"] and set(deg.tolist()) <= set(ip.DEGREES) and deg[-1] > 0
    assert n_rows < 17 or set(deg.tolist()) == set(ip.DEGREES)
    assert n_rows == 1 or not np.array_equal(np.argsort(case["src"].numpy(), kind="stable"), np.arange(deg.sum()))
    score, max_sim, max_eid, seg = ip.reference(case, None)
    slot = [int((case["src"][:e] == r).sum()) if d else -1 for r, (e, d) in enumerate(zip(max_eid.tolist(), deg))]
    assert slot == case["winner_slot"]
    where = {("first" if w == 0 else "last" if w == d - 1 else "middle") for w, d in zip(slot, deg) if d > 2}
    assert n_rows < 17 or where == {"first", "last", "middle"}
    assert bool((seg[deg > 0] >= 1000).all()) and bool((seg[deg == 0] == -1).all())
    # the second threshold splits the rows (one row: it passes)
    split = ip.reference(case, case["thresholds"][1])[3]
    assert bool((split[deg > 0] != -1).any()) and (n_rows < 5 or bool((split[deg > 0] == -1).any()))


def test_the_generic_routes_cover_every_degree_between_them():
    seen = set()
    for c in ip.GENERIC_CHANNELS:
        seen |= set(ip.designed_case(c, 5, torch.float32)["degrees"])
    assert seen == set(ip.DEGREES)
    assert all(ip.designed_case(c, 1, torch.float32)["degrees"][0] > 0 for c in ip.GENERIC_CHANNELS + tuple(ip.ROWS_PER_BLOCK))


@pytest.mark.parametrize("dtype", ip.DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("channels", sorted({c for _, c, _ in ip.routes()}))
def test_planted_case_is_certified_and_exact(dtype, channels):
    case = ip.planted_case(channels, dtype)
    assert ip.certify(case) >= ip.MIN_GAP
    src, di = case["src"], case["dst_index"]
    score, max_sim, max_eid, seg = ip.reference(case, None)
    slot = [int((src[:e] == r).sum()) if e < src.numel() else -1 for r, e in enumerate(max_eid.tolist())]
    assert slot == case["winner_slot"]                                   # duplicates, all-zero rows: the lowest edge id
    assert max_sim[ip.ROW_NEG] <= -2 * ip.MIN_GAP and bool((score[src == ip.ROW_NEG] < 0).all()) and seg[ip.ROW_NEG] >= 1000
    for r in (ip.ROW_ZERO_SRC, ip.ROW_ZERO_DST):
        assert bool((score[src == r] == 0).all()) and (src == r).sum() >= 3
    assert seg[ip.ROW_ZERO_SRC] == di[5] and seg[ip.ROW_ZERO_DST] == di[ip.COL_ZERO_B]
    assert sorted(score[src == ip.ROW_HOT_1].tolist()) == [-1.0, 0.0, 1.0] and sorted(score[src == ip.ROW_HOT_0].tolist()) == [-1.0, 0.0]
    assert score[src == ip.ROW_HOT_M1].tolist() == [-1.0]
    assert max_sim[[ip.ROW_HOT_1, ip.ROW_HOT_0, ip.ROW_HOT_M1]].tolist() == [1.0, 0.0, -1.0]
    assert bool((seg[: ip.ROW_EMPTY] >= 1000).all()) and seg[ip.ROW_EMPTY] == -1 and max_eid[ip.ROW_EMPTY] == src.numel()
    assert case["thresholds"] == (None, 0.0, 1.0, ip.ONE_UP) and np.float32(ip.ONE_UP) == ip.ONE_UP > 1.0
    on = {t: (ip.reference(case, t)[3] != -1).tolist() for t in case["thresholds"][1:]}
    #            dup    neg    zero_src zero_dst hot_1 hot_0  hot_m1 empty
    assert on[0.0][1:] == [False, True, True, True, True, False, False] and on[0.0][0] == bool(max_sim[ip.ROW_DUP] > 0)
    assert on[1.0] == [False, False, False, False, True, False, False, False]
    assert on[ip.ONE_UP] == [False] * 8
