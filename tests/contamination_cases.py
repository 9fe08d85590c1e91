"""Cases and CPU oracles for the contamination scoring (``segger_amd.validation``, ``csrc/contamination.hip``).

The oracles are float64 numpy restatements of the reference's ``src/segger/validation/contamination.py``:
``get_neighbor_frequencies`` (scipy ``cKDTree``, the cell itself included, as cuML's ``kneighbors`` on its own training
set), ``calculate_contamination``, ``contamination_flow`` and ``expression_summary_from_anndata``, with the two deviations
``segger_amd/validation.py`` states (a cell with no type gets ``P_self = eps``; an unlabelled neighbour is skipped) and the
sums over the types in float64, where the reference multiplies in float32.

The reference module itself cannot be imported here: cupy, cuml, scanpy, anndata and polars are all absent.  The
restatement is therefore UNPINNED beyond scipy's own pieces (``cKDTree`` for the neighbours, ``scipy.sparse.csr_matrix``
for the frequency table, which tests/test_contamination_cases.py compares against); everything else is checked by hand-
computed values there.

Two margins are conditions on the INPUTS, asserted by :func:`check_margins` for every case, every row and every entry:

* the k-th and (k + 1)-th neighbour distances of every cell differ by more than ``DIST_TOL`` (relative), far above the
  float32 rounding of a distance of float32-exact coordinates (2^-23), and no distance among the k nearest is within
  ``DIST_TOL`` of ``max_distance`` -- so the float32 search on the device and the float64 ``cKDTree`` pick the same cells;
* no entry has ``|q_self - cutoff| < 1e-6`` in the oracle -- so the flag does not hang on the last bits.

Seeds are searched on the CPU (:func:`make_case` tries consecutive seeds) until both hold for everything; no case leaves
any row or entry out."""
import numpy as np
from scipy.spatial import cKDTree

DIST_TOL = 1e-4
Q_MARGIN = 1e-6
ROW_LENGTHS = (0, 1, 63, 64, 65, 200)          # the first rows of every case with enough cells; then a row of missing genes
N_COLS = 256

#        name            n    T   G_ref  k   max_distance  extra
SPECS = [("t1_k1",       150, 1,   7,    1,  None,  {}),
         ("t3_maxdist",  300, 3,   70,   10, 20.0,  {"unlabelled": 0.15, "isolated": True}),
         ("t3_g600",     200, 3,   600,  7,  None,  {"unlabelled": 0.1}),
         ("t33_g600",    250, 33,  600,  10, 30.0,  {"unlabelled": 0.05}),
         ("t64_k_is_n",  48,  64,  70,   48, None,  {}),
         ("t65_no_back", 200, 65,  7,    5,  25.0,  {"alpha_background": 0.0, "unlabelled": 0.1}),
         ("t256_g70",    220, 256, 70,   16, None,  {"unlabelled": 0.05}),
         ("t256_g7",     160, 256, 7,    3,  15.0,  {"isolated": True})]


# ------------------------------------------------------------------ oracles ---
def neighbor_frequencies_oracle(xy, labels, k, n_types, max_distance=None):
    """-> (freq float32 [n, T], counts int32 [n, T]); ``labels`` -1 = unlabelled (skipped, never counted)"""
    xy = np.asarray(xy, dtype=np.float64)
    n = xy.shape[0]
    dist, idx = cKDTree(xy).query(xy, k=k)
    dist, idx = dist.reshape(n, k), idx.reshape(n, k)
    counts = np.zeros((n, n_types), dtype=np.int32)
    for i in range(n):
        for d, j in zip(dist[i], idx[i]):
            if j < n and (max_distance is None or d <= max_distance) and labels[j] >= 0:
                counts[i, labels[j]] += 1
    sums = counts.sum(1).astype(np.float64)
    inv = np.where(sums > 0, 1.0 / np.where(sums > 0, sums, 1.0), 0.0)
    return (counts.astype(np.float64) * inv[:, None]).astype(np.float32), counts


def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def contamination_oracle(indptr, indices, counts, gene_map, host_type, freq, weight, alpha_self=0.8, alpha_neighbor=0.15,
                         alpha_background=0.05, eps=1e-6, contam_cutoff=0.5):
    """float64 ``calculate_contamination`` after the frequencies: ``freq`` float32 [n, T], ``weight`` [T, G_ref]"""
    n, T = len(indptr) - 1, weight.shape[0]
    lik = (weight.astype(np.float32) + np.float32(eps)).astype(np.float64)            # the reference's float32 L
    rows = rows_of(indptr)
    g = gene_map[indices]
    missing = g < 0
    gs = np.where(missing, 0, g)
    kind = host_type[rows]
    labelled = host_type[host_type >= 0]
    share = np.bincount(labelled, minlength=T).astype(np.float64) / max(len(labelled), 1)
    back = share @ lik
    p_self = np.where(kind >= 0, lik[np.where(kind >= 0, kind, 0), gs], eps)
    nv = freq[rows].astype(np.float64)
    has = kind >= 0
    nv[np.nonzero(has)[0], kind[has]] = 0.0
    p_neigh = (nv * lik[:, gs].T).sum(axis=1) + eps
    p_back = back[gs] + eps
    q_self, q_neigh, q_back = alpha_self * p_self, alpha_neighbor * p_neigh, alpha_background * p_back
    denom = q_self + q_neigh + q_back
    q_self, q_neigh, q_back = q_self / denom, q_neigh / denom, q_back / denom
    for q in (q_self, q_neigh, q_back):
        q[missing] = 0.0
    flag = (q_self < contam_cutoff) & ~missing
    contamination = np.where(flag, counts, 0).astype(np.int32)
    contaminated = np.bincount(rows, weights=contamination, minlength=n).astype(np.int64)
    total = np.bincount(rows, weights=counts, minlength=n).astype(np.int64)
    return {"q_self": q_self, "q_neighbor": q_neigh, "q_background": q_back, "contamination": contamination,
            "contaminated": contaminated, "total": total, "missing": missing,
            "percent_contamination": 100.0 * contaminated / np.maximum(total, 1)}


def flow_oracle(indptr, indices, counts, contamination, gene_map, host_type, weight, n_host_types=None):
    """``contamination_flow`` -> [D, H] float64; raises ValueError when the table shares no gene with the matrix"""
    D = weight.shape[0]
    H = D if n_host_types is None else n_host_types
    if not np.any(gene_map >= 0):
        raise ValueError("No shared genes between the count matrix and the reference table")
    W = weight.astype(np.float64).T.copy()
    row_sum = W.sum(1, keepdims=True)
    row_sum[row_sum == 0] = 1.0
    W /= row_sum
    n = len(indptr) - 1
    rows = rows_of(indptr)
    g = gene_map[indices]
    keep = g >= 0
    contrib = np.zeros((n, D))
    np.add.at(contrib, rows[keep], contamination[keep, None].astype(np.float64) * W[g[keep]])
    libsize = np.bincount(rows, weights=counts, minlength=n)
    percent = 100.0 * contrib / np.maximum(libsize, 1.0)[:, None]
    flow = np.zeros((D, H))
    for h in range(H):
        members = host_type == h
        if members.any():
            flow[:, h] = percent[members].sum(0) / members.sum()
    return flow


def reference_table_oracle(indptr, indices, counts, cell_type, n_types, n_genes, min_counts=2):
    """``expression_summary_from_anndata`` -> n, me, pc, n_cells, weight (dense [T, G] tables)"""
    rows = rows_of(indptr)
    total = np.bincount(rows, weights=counts, minlength=len(indptr) - 1)
    value = np.log1p(counts.astype(np.float64) / (total / 1e4)[rows])
    kind = cell_type[rows]
    keep = (counts >= min_counts) & (kind >= 0) & (value > 0)
    n = np.zeros((n_types, n_genes), dtype=np.int64)
    s = np.zeros((n_types, n_genes))
    np.add.at(n, (kind[keep], indices[keep]), 1)
    np.add.at(s, (kind[keep], indices[keep]), value[keep])
    cells = np.bincount(cell_type[cell_type >= 0], minlength=n_types).astype(np.int64)
    me = np.where(n > 0, s / np.maximum(n, 1), 0.0)
    pc = np.where(n > 0, n / np.maximum(cells, 1)[:, None], 0.0)
    return {"n": n, "me": me, "pc": pc, "n_cells": cells, "weight": pc * me}


# ------------------------------------------------------------------ cases ---
def _build(name, n, T, G_ref, k, max_distance, extra, seed):
    rng = np.random.default_rng(seed)
    xy = np.round(rng.uniform(0.0, 120.0, size=(n, 2)) * 16.0) / 16.0                   # float32-exact coordinates
    labels = rng.integers(0, T, size=n).astype(np.int32)
    if n >= 40 and 2 <= k < n:                                                           # duplicate coordinates, one label each
        for a, b in ((10, 11), (20, 21), (30, 31)):
            xy[b] = xy[a]
            labels[b] = labels[a]
    if extra.get("isolated"):
        xy[n - 1] = (5000.0, 5000.0)                                                  # nothing within max_distance but itself
    if extra.get("unlabelled"):
        labels[rng.random(n) < extra["unlabelled"]] = -1
        labels[n - 1] = max(labels[n - 1], 0)
    gene_map = rng.integers(0, G_ref, size=N_COLS).astype(np.int32)
    gene_map[rng.random(N_COLS) < 0.12] = -1
    gene_map[:4] = -1                                                                 # the columns of the all-missing row
    gene_map[4] = 0
    lengths = rng.integers(3, 40, size=n)
    if n >= 40:
        lengths[:len(ROW_LENGTHS)] = ROW_LENGTHS
    indices, missing_row = [], len(ROW_LENGTHS)
    for r in range(n):
        if r == missing_row:
            cols = np.arange(4)
        else:
            cols = np.sort(rng.choice(N_COLS, size=lengths[r], replace=False))
        indices.append(cols)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in indices])]).astype(np.int64)
    indices = np.concatenate(indices).astype(np.int32)
    counts = rng.integers(1, 9, size=len(indices)).astype(np.int32)
    weight = rng.gamma(0.7, 1.0, size=(T, G_ref)) * (rng.random((T, G_ref)) < 0.7)
    weight[:, G_ref - 1] = 0.0                                                        # a gene no type expresses
    case = {"name": name, "seed": seed, "xy": xy, "labels": labels, "k": k, "n_types": T, "max_distance": max_distance,
            "indptr": indptr, "indices": indices, "counts": counts, "gene_map": gene_map, "weight": weight,
            "params": {"alpha_self": 0.8, "alpha_neighbor": 0.15, "alpha_background": extra.get("alpha_background", 0.05),
                       "eps": 1e-6, "contam_cutoff": 0.5}}
    return case


def distance_margins_hold(case):
    xy, k, n = case["xy"], case["k"], len(case["xy"])
    dist, _ = cKDTree(xy).query(xy, k=min(k + 1, n))
    dist = dist.reshape(n, -1)
    if k < n:
        gap = dist[:, k] - dist[:, k - 1]
        if not np.all(gap > DIST_TOL * np.maximum(dist[:, k], 1.0)):
            return False
    if case["max_distance"] is not None:
        md = case["max_distance"]
        if np.any(np.abs(dist[:, :k] - md) <= DIST_TOL * md):
            return False
    return True


def oracle_of(case):
    """every expected output of a case (computed from the inputs alone)"""
    freq, counts = neighbor_frequencies_oracle(case["xy"], case["labels"], case["k"], case["n_types"], case["max_distance"])
    out = contamination_oracle(case["indptr"], case["indices"], case["counts"], case["gene_map"], case["labels"], freq,
                               case["weight"], **case["params"])
    out["freq"], out["counts"] = freq, counts
    out["flow"] = flow_oracle(case["indptr"], case["indices"], case["counts"], out["contamination"], case["gene_map"],
                              case["labels"], case["weight"])
    return out


def q_margin_holds(case, oracle):
    known = ~oracle["missing"]
    return bool(np.all(np.abs(oracle["q_self"][known] - case["params"]["contam_cutoff"]) >= Q_MARGIN))


def check_margins(case, oracle):
    assert distance_margins_hold(case), case["name"]
    assert q_margin_holds(case, oracle), case["name"]


def make_case(spec):
    """the first seed (from a base fixed per case) at which both margins hold for every row and entry"""
    name, n, T, G_ref, k, max_distance, extra = spec
    base = 1000 * (1 + [s[0] for s in SPECS].index(name))
    for seed in range(base, base + 200):
        case = _build(name, n, T, G_ref, k, max_distance, extra, seed)
        if not distance_margins_hold(case):
            continue
        oracle = oracle_of(case)
        if q_margin_holds(case, oracle):
            return case, oracle
    raise AssertionError(f"{name}: no seed keeps both margins")


_CACHE = {}


def cases():
    """name -> (case, oracle), built once per process and never modified"""
    if not _CACHE:
        for spec in SPECS:
            _CACHE[spec[0]] = make_case(spec)
    return _CACHE


# ------------------------------------------------------------------ synthetic tissue ---
TISSUE_GENES = 20


def tissue(n_cells, seed, mean_count=5.0):
    """A two-type tissue of doublets as a transcript table: cells sit in pairs (one of each type, 4 apart, the pairs on a
    jittered lattice of pitch 16), so every cell's nearest cell of the other type is its partner; type 0 expresses genes
    0-9, type 1 genes 10-19 (and a trace of the other half).  -> dict(xy [n, 2], kind [n], tx_cell, tx_home, tx_gene):
    one row per transcript, ``tx_cell`` the cell it is assigned to and ``tx_home`` the cell it lies in."""
    rng = np.random.default_rng(seed)
    n_pairs = (n_cells + 1) // 2
    side = int(np.ceil(np.sqrt(n_pairs)))
    grid = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n_pairs].astype(np.float64)
    centre = grid * 16.0 + rng.uniform(-2.0, 2.0, size=grid.shape)
    angle = rng.uniform(0.0, 2.0 * np.pi, size=n_pairs)
    arm = 2.0 * np.stack([np.cos(angle), np.sin(angle)], -1)
    xy = np.round(np.concatenate([centre + arm, centre - arm])[:n_cells] * 16.0) / 16.0
    kind = np.concatenate([np.zeros(n_pairs, np.int32), np.ones(n_pairs, np.int32)])[:n_cells]
    own = np.zeros((2, TISSUE_GENES))
    own[0, :10], own[1, 10:] = mean_count, mean_count
    own += 0.05
    dense = rng.poisson(own[kind])
    cell, gene = np.nonzero(dense)
    reps = dense[cell, gene]
    tx_cell = np.repeat(cell, reps).astype(np.int32)
    return {"xy": xy, "kind": kind, "tx_cell": tx_cell, "tx_home": tx_cell.copy(), "tx_gene": np.repeat(gene, reps).astype(np.int32)}


def swap_fraction(t, fraction=0.2):
    """move ``floor(fraction * count)`` transcripts of every (cell, gene) to the nearest cell of the OTHER type"""
    xy, kind = t["xy"], t["kind"]
    nearest_other = np.empty(len(xy), dtype=np.int64)
    for a in (0, 1):
        others = np.nonzero(kind != a)[0]
        _, j = cKDTree(xy[others]).query(xy[kind == a], k=1)
        nearest_other[kind == a] = others[j]
    key = t["tx_cell"].astype(np.int64) * TISSUE_GENES + t["tx_gene"]
    order = np.argsort(key, kind="stable")
    key = key[order]
    start = np.r_[0, np.nonzero(np.diff(key))[0] + 1]
    length = np.diff(np.r_[start, len(key)])
    rank = np.arange(len(key)) - np.repeat(start, length)
    moved = rank < np.repeat(np.floor(fraction * length).astype(np.int64), length)
    cell = t["tx_cell"][order].copy()
    cell[moved] = nearest_other[cell[moved]]
    return {"xy": xy, "kind": kind, "tx_cell": cell.astype(np.int32), "tx_home": t["tx_cell"][order], "tx_gene": t["tx_gene"][order]}


def tissue_csr(t):
    """canonical CSR of the transcript table (every cell present) -> indptr int64, indices int32, counts int32"""
    n = len(t["xy"])
    key, counts = np.unique(t["tx_cell"].astype(np.int64) * TISSUE_GENES + t["tx_gene"], return_counts=True)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(key // TISSUE_GENES, minlength=n))
    return indptr, (key % TISSUE_GENES).astype(np.int32), counts.astype(np.int32)


def tissue_scores(t, labels, k=10, max_distance=20.0):
    """the oracle chain on a tissue with the given labels: table from the same matrix -> contamination -> flow"""
    indptr, indices, counts = tissue_csr(t)
    T = int(labels.max()) + 1
    table = reference_table_oracle(indptr, indices, counts, labels, T, TISSUE_GENES)
    freq, _ = neighbor_frequencies_oracle(t["xy"], labels, k, T, max_distance)
    gene_map = np.arange(TISSUE_GENES, dtype=np.int32)
    out = contamination_oracle(indptr, indices, counts, gene_map, labels, freq, table["weight"])
    out["flow"] = flow_oracle(indptr, indices, counts, out["contamination"], gene_map, labels, table["weight"])
    return out
