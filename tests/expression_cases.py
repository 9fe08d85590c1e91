"""Shared by the expression-matrix tests: the CPU oracle of ``postprocess.expression_matrix`` and the case generators.

The reference builds the matrix in ``anndata_from_transcripts`` (``src/segger/data/utils/anndata.py:18-102``): a polars
group-by on (cell, gene), then ``scipy.sparse.coo_matrix((counts, (cell_pos, gene_pos))).tocsr()``.  That function cannot
run here (polars and scanpy are absent), so nothing is taken from it but that one scipy call: the oracle filters the rows
(``writer.py:97-99`` plus the ``is_not_null`` of ``anndata.py:28``), orders them with ``np.lexsort``, reduces with
``np.add.reduceat`` in float64 and builds ``X`` by literally that call, one ``1`` per kept row (``tocsr`` sums the
duplicates).  The axes are ascending ids, this project's documented choice."""
import numpy as np
import scipy.sparse as sp
import torch

EPS = 2.0 ** -52


def expression_oracle(cell, gene, sim, thr, xy=None):
    """-> dict of numpy arrays named like the outputs of ``expression_matrix`` plus ``dense`` (the count matrix),
    ``n_max_run`` / ``n_max_cell`` (the longest sum of a mean / of a centroid) and ``n_kept``."""
    cell = np.asarray(cell, dtype=np.int64)
    gene = np.asarray(gene, dtype=np.int64)
    sim = np.asarray(sim, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        keep = (cell >= 0) & (sim.astype(np.float64) >= thr)          # a NaN on either side compares false
    rows = np.flatnonzero(keep)
    c, g, s = cell[rows], gene[rows], sim[rows].astype(np.float64)
    cell_ids, gene_ids = np.unique(c), np.unique(g)
    cp, gp = np.searchsorted(cell_ids, c), np.searchsorted(gene_ids, g)
    shape = (cell_ids.size, gene_ids.size)
    X = sp.coo_matrix((np.ones(rows.size, dtype=np.int32), (cp, gp)), shape=shape).tocsr()      # the reference's call
    X.sort_indices()
    order = np.lexsort((rows, gp, cp))                                # by cell, then gene, then row position
    pair = cp[order] * max(gene_ids.size, 1) + gp[order]
    heads = np.flatnonzero(np.r_[True, pair[1:] != pair[:-1]]) if rows.size else np.zeros(0, dtype=np.int64)
    run_len = np.diff(np.r_[heads, rows.size])
    mean = np.add.reduceat(s[order], heads) / run_len if rows.size else np.zeros(0)
    cell_count = np.bincount(cp, minlength=cell_ids.size).astype(np.int64)
    out = {"cell_ids": cell_ids.astype(np.int32), "gene_ids": gene_ids.astype(np.int32), "indptr": X.indptr.astype(np.int64),
           "indices": X.indices.astype(np.int32), "counts": X.data.astype(np.int32), "mean_similarity": mean,
           "cell_count": cell_count, "dense": X.toarray(), "n_kept": int(rows.size),
           "n_max_run": int(run_len.max()) if rows.size else 0, "n_max_cell": int(cell_count.max()) if rows.size else 0}
    assert np.array_equal(run_len, out["counts"])                     # the group-by and the scipy call agree
    if xy is not None:
        p = np.asarray(xy, dtype=np.float32).astype(np.float64)[rows][order]
        cheads = np.flatnonzero(np.r_[True, cp[order][1:] != cp[order][:-1]]) if rows.size else np.zeros(0, dtype=np.int64)
        out["centroid"] = (np.add.reduceat(p, cheads, axis=0) / cell_count[:, None]) if rows.size else np.zeros((0, 2))
    return out


def make_case(cell, gene, sim, thr, xy=True, n_cells=None, n_genes=None, seed=0):
    """A case = the deduplicated columns of a slide in ascending row_index (numpy), with seeded positions."""
    cell = np.asarray(cell, dtype=np.int64)
    n = cell.size
    case = {"cell": cell, "gene": np.asarray(gene, dtype=np.int64), "sim": np.asarray(sim, dtype=np.float32),
            "thr": np.asarray(thr, dtype=np.float64), "n_cells": n_cells, "n_genes": n_genes, "xy": None}
    if xy:
        case["xy"] = np.random.default_rng(seed + 1000).uniform(0.0, 4096.0, (n, 2)).astype(np.float32)
    return case


def runs_case(run_lengths, seed, not_kept=0.0, n_cells=None, n_genes=None):
    """One (cell, gene) pair per entry of ``run_lengths`` with that many kept rows (pairs walk a 5-gene grid), the rows
    shuffled over the slide; a fraction ``not_kept`` of extra rows fails the filter one way or another."""
    rng = np.random.default_rng(seed)
    cell = np.concatenate([np.full(m, i // 5) for i, m in enumerate(run_lengths)])
    gene = np.concatenate([np.full(m, (3 * i) % 5) for i, m in enumerate(run_lengths)])
    n = cell.size
    sim = rng.uniform(0.25, 1.0, n).astype(np.float32)
    thr = np.full(n, 0.25)
    extra = int(round(not_kept * n))
    if extra:
        e_cell = rng.integers(-1, cell.max() + 1, extra)
        e_gene = rng.integers(0, 5, extra)
        e_sim = rng.uniform(-1.0, 0.2, extra).astype(np.float32)
        cell, gene, sim = np.r_[cell, e_cell], np.r_[gene, e_gene], np.r_[sim, e_sim]
        thr = np.r_[thr, np.where(rng.random(extra) < 0.2, np.nan, 0.25)]
    p = rng.permutation(cell.size)
    return make_case(cell[p], gene[p], sim[p], thr[p], n_cells=n_cells, n_genes=n_genes, seed=seed)


def random_case(n, n_cells, n_genes, seed):
    """``n`` rows over ``n_cells`` x ``n_genes``: a tenth unassigned, per-gene thresholds (one gene without: NaN),
    similarities in [-1, 1] with a quarter rounded to 1/64 so that ``sim == thr`` occurs."""
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, n_cells, n)
    cell[rng.random(n) < 0.1] = -1
    gene = rng.integers(0, n_genes, n)
    sim = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    sim[::4] = np.round(sim[::4] * 64) / 64
    gene_thr = np.round(rng.uniform(0.0, 0.5, n_genes) * 64) / 64
    gene_thr[n_genes // 2] = np.nan
    return make_case(cell, gene, sim, gene_thr[gene], n_cells=n_cells, n_genes=n_genes, seed=seed)


def as_result(case, device):
    """The dict ``assign_transcripts_to_cells`` returns, on ``device``; row_index = the row's position."""
    n = case["cell"].size
    return {"row_index": torch.arange(n, device=device),
            "cell_encoding": torch.from_numpy(case["cell"]).to(device),
            "gene": torch.from_numpy(case["gene"]).to(device),
            "similarity": torch.from_numpy(case["sim"]).to(device),
            "similarity_threshold": torch.from_numpy(case["thr"]).to(device)}


def case_oracle(case):
    return expression_oracle(case["cell"], case["gene"], case["sim"], case["thr"], case["xy"])


INT_KEYS = ("cell_ids", "gene_ids", "indptr", "indices", "counts", "cell_count")


def assert_matches_oracle(got, want, max_sim=1.0, max_coord=None):
    """Exact integer outputs; means and centroids within the float64 summation-order bound of the case.  A sum of n
    terms of magnitude <= v, in any order, is within (n - 1) 2^-53 n v of the exact sum, so its mean within (n - 1) 2^-53 v,
    plus one rounding of the division, 2^-53 v: two means of the same run differ by at most 2 n 2^-53 v = n 2^-52 v, with n
    the longest run of the case and v = 1 >= |sim|.  The centroids are held to the same n with v the largest |coordinate|:
    tighter than the worst case of a cell of several runs (its sum has more terms), and still far above what float64 sums
    of fp32 coordinates lose."""
    for k in INT_KEYS:
        w = torch.from_numpy(want[k])
        assert got[k].dtype == w.dtype and torch.equal(got[k].cpu(), w), k
    assert got["n_kept"] == want["n_kept"]
    g = got["mean_similarity"].cpu()
    assert g.dtype == torch.float64 and g.shape == (want["mean_similarity"].size,)
    if g.numel():
        err = float((g - torch.from_numpy(want["mean_similarity"])).abs().max())
        bound = want["n_max_run"] * EPS * max_sim
        print(f"mean_similarity: max |err| {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    if "centroid" in want:
        c = got["centroid"].cpu()
        assert c.dtype == torch.float64 and c.shape == want["centroid"].shape
        if c.numel():
            err = float((c - torch.from_numpy(want["centroid"])).abs().max())
            bound = want["n_max_run"] * EPS * max_coord
            print(f"centroid: max |err| {err:.3e}, bound {bound:.3e}")
            assert err <= bound
    else:
        assert "centroid" not in got
