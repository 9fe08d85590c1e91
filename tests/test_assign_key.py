"""The packed (similarity, arrival order) key of the streaming assignment (include/segger_amd.h, segger_assign_update),
restated in numpy: ordering rows by key, descending, is ``postprocess.best_assignment``'s order -- similarity descending
with NaN on top, stable, so the first row of the concatenation wins a tie (and +-0 is a tie).  No GPU."""
import numpy as np
import torch

from segger_amd import postprocess as pp

from assign_cases import assign_keys, key_test_similarities, special_similarities


def winners(sim, groups):
    """best_assignment over rows (in concatenation order) grouped into transcripts -> winning row id per transcript."""
    n = len(sim)
    out = pp.best_assignment([(torch.from_numpy(groups.astype(np.int64)), torch.arange(n), torch.from_numpy(sim),
                               torch.zeros(n, dtype=torch.int32))])
    return out["row_index"].numpy(), out["cell_encoding"].numpy()


def test_key_order_is_best_assignments_order():
    sim = key_test_similarities()
    n = sim.size
    assert n >= 2000 and np.isnan(sim).sum() == 6 and (sim == 0).sum() >= 4
    keys = assign_keys(sim, np.arange(n))
    assert len(np.unique(keys)) == n
    order = np.argsort(keys)[::-1]                                   # keys are unique: no tie to break
    # the order best_assignment sorts by, directly
    assert np.array_equal(order, torch.sort(torch.from_numpy(sim), descending=True, stable=True).indices.numpy())
    # ... and through best_assignment itself: transcript k holds the rows of rank k and k + 1, in arrival order; the
    # winner must be the row of rank k, for every k (adjacent pairs pin the whole order down)
    pair = np.stack([order[:-1], order[1:]], 1)
    pair.sort(1)                                                     # arrival order inside a transcript
    rows = pair.reshape(-1)
    tx, seg = winners(sim[rows], np.repeat(np.arange(n - 1), 2))
    assert np.array_equal(tx, np.arange(n - 1)) and np.array_equal(rows[seg], order[:-1])
    # random transcripts of ~40 rows each: the winner is the row of the largest key
    rng = np.random.default_rng(1)
    groups = rng.integers(0, 50, n)
    tx, seg = winners(sim, groups)
    want = np.array([np.flatnonzero(groups == g)[np.argmax(keys[groups == g])] for g in tx])
    assert np.array_equal(seg, want)


def test_ties_nan_and_zero_signs():
    s = special_similarities()
    k = assign_keys(s, np.zeros(s.size))
    name = dict(zip(["p0", "n0", "p1", "n1", "pinf", "ninf", "nan", "nnan", "nan_payload", "pden", "nden", "pden2", "nden2"], k))
    assert name["p0"] == name["n0"] and name["nan"] == name["nnan"] == name["nan_payload"]
    assert (name["nan"] > name["pinf"] > name["p1"] > name["pden2"] > name["pden"] > name["p0"] > name["nden"]
            > name["nden2"] > name["n1"] > name["ninf"])
    # at equal similarity the earlier row has the larger key
    assert assign_keys([0.5], [3])[0] > assign_keys([0.5], [4])[0]
    assert assign_keys([0.5], [2 ** 32 - 1])[0] < assign_keys([np.nextafter(np.float32(0.5), np.float32(1))], [0])[0]


def test_no_real_key_is_zero():
    sim = np.concatenate([key_test_similarities(), special_similarities()])
    for q in (0, 1, 2 ** 31, 2 ** 32 - 1):
        assert (assign_keys(sim, np.full(sim.size, q)) != 0).all()
    # the smallest key of all: -NaN would map to ord 0, and is canonicalised away; -inf at the last sequence number
    assert assign_keys([-np.inf], [2 ** 32 - 1])[0] == np.uint64(0x007FFFFF) << np.uint64(32)
