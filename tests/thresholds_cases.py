"""Inputs of the per-gene threshold tests (no GPU, plain numpy), their float64 reference, and the certificate that every
input is well-conditioned for that reference.

A case is ``{"sim": float32 [n], "gene": int32 [n], "cell": int32 [n], "n_genes": int, "max_iter": int}``.  The
reference is ``oracle/postprocess_oracle.py`` gene by gene: ``threshold_yen``, ``threshold_li``, the median back-fill.

Li's fixed point and Yen's argmax may legitimately branch on a last-bit difference (another ``log``, another summation
order), so :func:`certify` demands of every committed case, for the float64 oracle alone, that

* every Li iterate ``t`` stays more than ``MARGIN`` away from the nearest (shifted) data value, so that no ``a > t``
  comparison can flip, and
* Yen's winning criterion exceeds every other by more than ``MARGIN`` relative, or ties it exactly.

A case that fails is replaced by another seed here, never excused in a GPU test: this is a condition on the inputs, not a
tolerance on the kernel.  :func:`li_trace` is the instrumented copy of the oracle's Li loop; :func:`certify` also asserts
that it agrees with ``threshold_li`` itself."""
import numpy as np

from segger_amd._lib import THRESHOLDS_CHUNK as CHUNK

MARGIN = 1e-9
SIZES = (1, 2, 63, 64, 65, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
LARGE = 300_000


def bimodal(rng, n):
    """The similarities of tests/test_postprocess.py::fake_predictions: assigned-well vs noise."""
    hi = rng.random(n) < 0.6
    v = np.where(hi, 0.7 + 0.1 * rng.standard_normal(n), 0.1 + 0.15 * rng.standard_normal(n))
    return np.clip(v, -1.0, 1.0).astype(np.float32)


def make_case(genes, n_genes=None, max_iter=250, seed=0, unassigned=0):
    """``genes``: {gene id: float32 values of its assigned rows}.  ``unassigned`` extra rows with cell = -1 (and genes and
    similarities of their own, which must change nothing) are mixed in, and the rows are shuffled."""
    rng = np.random.default_rng(seed)
    ids = sorted(genes)
    sim = np.concatenate([np.asarray(genes[g], dtype=np.float32) for g in ids] + [bimodal(rng, unassigned)])
    gene = np.concatenate([np.full(len(genes[g]), g, dtype=np.int32) for g in ids]
                          + [rng.integers(0, max(ids) + 1, unassigned).astype(np.int32)])
    cell = np.concatenate([rng.integers(0, 50, sim.size - unassigned), np.full(unassigned, -1)]).astype(np.int32)
    order = rng.permutation(sim.size)
    return {"sim": sim[order], "gene": gene[order], "cell": cell[order],
            "n_genes": int(max(ids) + 1 if n_genes is None else n_genes), "max_iter": max_iter}


def slide_case(seed, n_genes=12, max_iter=250):
    """The deduplicated rows of a seeded slide of tests/test_postprocess.py."""
    import postprocess_oracle as po
    from test_postprocess import fake_predictions
    ref = po.assign_transcripts_to_cells([[t.numpy() for t in p] for p in fake_predictions(seed, n_genes=n_genes)], max_iter)
    return {"sim": ref["similarity"].astype(np.float32), "gene": ref["gene"].astype(np.int32),
            "cell": ref["cell_encoding"].astype(np.int32), "n_genes": n_genes, "max_iter": max_iter}


def sizes_case():
    rng = np.random.default_rng(11)
    return make_case({g: bimodal(rng, n) for g, n in enumerate(SIZES)}, seed=12, unassigned=300)


def edge_case():
    rng = np.random.default_rng(21)
    z = np.float32(0.0)
    genes = {
        0: [0.4],                                                       # flat: one value
        2: [0.4] * 37,                                                  # flat: many equal values
        3: [0.25] * 5 + [0.5] * 3,                                      # exactly two distinct values
        5: [-z, z, z, -z, 0.25, 0.5, 0.5, 0.75, 1.0],                   # -0.0 and +0.0: two keys, one value
        6: [-z, z, -z],                                                 # ... and nothing else: flat
        9: np.repeat(np.arange(65) / 64.0, rng.integers(1, 6, 65)),     # every value on a bin edge of [0, 1]
        10: bimodal(rng, 500),
    }                                                                   # ids 1, 4, 7, 8 and 11..14 are absent
    return make_case(genes, n_genes=15, seed=22, unassigned=40)


def large_case():
    rng = np.random.default_rng(31)
    return make_case({0: bimodal(rng, 50), 1: bimodal(rng, LARGE), 2: bimodal(rng, 700), 4: bimodal(rng, 3)}, seed=32,
                     unassigned=1000)


def known_case():
    """The hand cases of tests/test_postprocess.py::test_known_answers: gene 0 -> min(0.5, 0.25 + 0.5 / 512), gene 1 flat."""
    return make_case({0: [0.25] * 10 + [0.75] * 10, 1: [0.4] * 5}, seed=41)


def all_cases():
    cases = {f"slide{seed}": slide_case(seed) for seed in (0, 1, 2)}
    cases["slide7_max_iter6"] = slide_case(7, n_genes=9, max_iter=6)
    cases.update(sizes=sizes_case(), edges=edge_case(), large=large_case(), known=known_case())
    return cases


def li_trace(arr, max_iter=250):
    """``postprocess_oracle.threshold_li`` with its iterates: -> (value, converged, [(t, distance to the nearest value)]).
    ``value`` of a failed gene is the last iterate (the oracle raises StopIteration there)."""
    a = np.asarray(arr, dtype=np.float64).ravel()
    if np.all(a == a[0]):
        return float(a[0]), True, []
    a_min = a.min()
    a = a - a_min
    tol = np.min(np.diff(np.unique(a))) / 2.0
    t_next = a.mean()
    t_curr = -2.0 * tol
    calls = 1
    trace = []
    while abs(t_next - t_curr) > tol:
        t_curr = t_next
        trace.append((float(t_curr), float(np.abs(a - t_curr).min())))
        fg = a > t_curr
        mean_fore = a[fg].mean()
        mean_back = a[~fg].mean()
        if mean_back == 0:
            break
        t_next = (mean_back - mean_fore) / (np.log(mean_back) - np.log(mean_fore))
        calls += 1
        if calls > max_iter:
            return float(t_next + a_min), False, trace
    return float(t_next + a_min), True, trace


def yen_criterion(arr, nbins=256):
    """The criterion ``postprocess_oracle.threshold_yen`` takes the argmax of."""
    a = np.asarray(arr, dtype=np.float64).ravel()
    lo, hi = a.min(), a.max()
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    counts, _ = np.histogram(a, bins=nbins, range=(lo, hi))
    pmf = counts.astype(np.float64) / counts.sum()
    p1 = np.cumsum(pmf)
    p1_sq = np.cumsum(pmf ** 2)
    p2_sq = np.cumsum(pmf[::-1] ** 2)[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(((p1_sq[:-1] * p2_sq[1:]) ** -1) * (p1[:-1] * (1.0 - p1[:-1])) ** 2)


def gene_values(case, g):
    return case["sim"][(case["gene"] == g) & (case["cell"] >= 0)]


def reference(case):
    """The oracle over the gene id domain: threshold (back-filled), yen, li (NaN for a failed gene: the oracle has no
    value there), count, converged, failed_genes, global_threshold."""
    import postprocess_oracle as po
    n = case["n_genes"]
    yen, li = np.full(n, np.nan), np.full(n, np.nan)
    count, conv = np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
    for g in range(n):
        arr = gene_values(case, g)
        count[g] = arr.size
        if arr.size == 0:
            continue
        yen[g] = po.threshold_yen(arr)
        try:
            li[g] = po.threshold_li(arr, case["max_iter"])
        except StopIteration:
            conv[g] = False
    thr = np.where(li < yen, li, yen)
    voted = conv & (count > 0)
    glob = float(np.quantile(thr[voted], 0.5)) if voted.any() else float("nan")
    thr = np.where(conv, thr, glob)
    return {"threshold": thr, "yen": yen, "li": li, "count": count, "converged": conv,
            "failed_genes": np.flatnonzero(~conv).astype(np.int64), "global_threshold": glob}


def certify(case):
    """Assert that ``case`` is well-conditioned for the float64 oracle; -> the smallest Li margin met (inf if none)."""
    import postprocess_oracle as po
    worst = np.inf
    for g in range(case["n_genes"]):
        arr = gene_values(case, g)
        if arr.size == 0:
            continue
        value, converged, trace = li_trace(arr, case["max_iter"])
        try:                                                            # the instrumented copy is the oracle's loop
            want = po.threshold_li(arr, case["max_iter"])
        except StopIteration:
            want = None
        assert (converged and value == want) if want is not None else not converged, g
        for t, margin in trace:
            assert margin > MARGIN, (g, t, margin)
            worst = min(worst, margin)
        crit = yen_criterion(arr)
        if np.isnan(crit).any():                                        # a product of exact zeros (empty leading bins)
            continue
        top = crit.max()
        rest = crit[crit != top]
        if rest.size and np.isfinite(top):
            assert rest.max() < top - MARGIN * abs(top), (g, top, rest.max())
    return worst
