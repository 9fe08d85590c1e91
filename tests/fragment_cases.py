"""CPU oracle and cases for segger_amd.fragments (numpy, scipy and torch on the CPU; no GPU).

:func:`oracle` is a SEQUENTIAL RESTATEMENT of the contract in include/segger_amd.h -- float64 cosine on the upcast stored
values, ``scipy.sparse.csgraph.connected_components`` on the kept edges, the min-size filter, canonical renumbering by
smallest member.  It is UNPINNED by any reference: upstream segger's fragment mode is not in the reference snapshot this
project follows, so there is no reference file to cite and no reference run to compare with.

The device decides ``sim >= min_similarity`` in fp32; the oracle in float64.  The two agree for every live edge whose exact
cosine is farther from the threshold than ``segger_amd.fragments.similarity_error_bound`` -- the oracle reports the smallest
distance (``margin``) and tests/test_host_fragments.py asserts that condition, on the CPU, for every case of
:data:`Z_CASES`, which is what lets tests/test_gpu_fragments.py demand equality."""
from collections import namedtuple

import numpy as np
import torch

Case = namedtuple("Case", "n unassigned batches min_similarity min_size first_id")
Batch = namedtuple("Batch", "z edge_index tx_index mask similarity keep", defaults=(None, None, None, None))


def _np(t):
    return None if t is None else t.numpy()


def oracle(case: Case) -> dict:
    """-> fragment, root, size (int64 arrays), the counters, ``parent`` (the smallest member of every transcript's
    component) and ``margin`` (the smallest |sim - threshold| over the live edges of the z batches; inf without one)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n = case.n
    un = case.unassigned.numpy().astype(bool)
    thr = float(np.float32(case.min_similarity))
    rows, cols = [], []
    n_edges = n_live = n_kept = n_bad = 0
    margin = float("inf")
    for b in case.batches:
        ei = b.edge_index.numpy().astype(np.int64)
        e = ei.shape[1]
        n_edges += e
        sizes = [int(t.shape[0]) for t in (b.z, b.tx_index, b.mask) if t is not None]
        n_nodes = sizes[0] if sizes else n
        s, d = ei
        ok = (s >= 0) & (s < n_nodes) & (d >= 0) & (d < n_nodes)
        bad = ~ok
        s0, d0 = np.where(ok, s, 0), np.where(ok, d, 0)
        consider = ok & (_np(b.mask)[s0] if b.mask is not None else True)
        ts, td = (_np(b.tx_index).astype(np.int64)[s0], _np(b.tx_index).astype(np.int64)[d0]) if b.tx_index is not None else (s0, d0)
        tok = (ts >= 0) & (ts < n) & (td >= 0) & (td < n)
        bad |= consider & ~tok
        consider &= tok
        ts0, td0 = np.where(consider, ts, 0), np.where(consider, td, 0)
        live = consider & un[ts0] & un[td0] & (ts0 != td0)
        if b.keep is not None:
            live &= _np(b.keep)
        n_bad += int(bad.sum())
        n_live += int(live.sum())
        if b.z is not None:
            zz = b.z.double().numpy()                                 # the stored values, upcast exactly
            a, c = zz[s0[live]], zz[d0[live]]
            dot, aa, bb = (a * c).sum(1), (a * a).sum(1), (c * c).sum(1)
            sim = dot / (np.maximum(np.sqrt(aa), 1e-8) * np.maximum(np.sqrt(bb), 1e-8))
            if sim.size:
                margin = min(margin, float(np.abs(sim - thr).min()))
        elif b.similarity is not None:
            sim = b.similarity.double().numpy()[live]
        else:
            sim = np.full(int(live.sum()), np.inf)
        kept = sim >= thr                                             # NaN: not kept
        n_kept += int(kept.sum())
        rows.append(ts0[live][kept])
        cols.append(td0[live][kept])
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    g = sp.coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    smallest = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(smallest, lab, np.arange(n))
    parent = smallest[lab]                                            # assigned transcripts are singletons: their own id
    members = np.bincount(parent[un], minlength=n)
    is_root = un & (parent == np.arange(n))
    flagged = is_root & (members >= case.min_size)
    root = np.nonzero(flagged)[0]
    rank = np.full(n, -1, np.int64)
    rank[root] = np.arange(root.size)
    fragment = np.where(un & (rank[parent] >= 0), case.first_id + rank[parent], -1)
    return {"fragment": fragment, "root": root, "size": members[root], "parent": parent, "margin": margin,
            "n_edges": n_edges, "n_live_edges": n_live, "n_kept_edges": n_kept, "n_bad": n_bad,
            "n_candidates": int(un.sum()), "n_components": int(is_root.sum()), "n_fragments": int(root.size)}


# ---------------------------------------------------------------------------------------------- builders ---
def ones_z(n, C=8, dtype=torch.float32):
    """every pair agrees (cosine 1 to rounding): the graph alone decides"""
    return torch.ones(n, C, dtype=dtype)


def edges(pairs):
    return torch.tensor(np.asarray(pairs, np.int64).reshape(-1, 2).T.copy())


def graph_case(n, pairs, unassigned=None, C=8, dtype=torch.float32, min_size=1, first_id=0, splits=1, mask=None):
    un = torch.ones(n, dtype=torch.bool) if unassigned is None else torch.as_tensor(np.asarray(unassigned, bool))
    ei = edges(pairs)
    z = ones_z(n, C, dtype)
    parts = np.array_split(np.arange(ei.shape[1]), splits)
    batches = [Batch(z, ei[:, torch.as_tensor(p)], None, mask) for p in parts]
    return Case(n, un, batches, 0.5, min_size, first_id)


def path_pairs(n, order, seed=0):
    p = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    if order == "descending":
        p = p[::-1]
    elif order == "shuffled":
        p = p[np.random.default_rng(seed).permutation(n - 1)]
    return p


def disjoint_pairs(E):
    """edge e joins nodes 2e and 2e + 1: E components of two"""
    return np.stack([2 * np.arange(E), 2 * np.arange(E) + 1], 1)


def binary_rows(dtype):
    """rows with entries in {0, 1}, four ones each: norm 2, cosines exactly k / 4.  Row 0 is the anchor; row k + 1 shares k ones."""
    z = torch.zeros(6, 8)
    z[0, :4] = 1
    for k in range(5):
        z[k + 1, 4 - k:8 - k] = 1
    return z.to(dtype)


def exact_threshold_case(dtype):
    """the anchor against rows sharing 0 .. 4 ones, both directions: at 0.5, k >= 2 is kept and k = 1 is not"""
    pairs = [(0, k + 1) for k in range(5)] + [(k + 1, 0) for k in range(5)]
    return Case(6, torch.ones(6, dtype=torch.bool), [Batch(binary_rows(dtype), edges(pairs))], 0.5, 1, 0)


def similarity_case():
    """the similarity route at the threshold, one ulp below and one ulp above; one pair whose two directions disagree"""
    thr = np.float32(0.5)
    lo, hi = np.nextafter(thr, np.float32(-1)), np.nextafter(thr, np.float32(2))
    pairs = [(0, 1), (2, 3), (4, 5), (6, 7), (7, 6), (8, 9), (9, 8)]
    sim = torch.tensor(np.array([thr, lo, hi, 0.6, 0.4, 0.4, np.nan], np.float32))
    return Case(10, torch.ones(10, dtype=torch.bool), [Batch(None, edges(pairs), similarity=sim)], 0.5, 1, 0)


def knn_pairs(xy, k):
    from scipy.spatial import cKDTree
    _, idx = cKDTree(xy).query(xy, k=k + 1)
    src = np.repeat(np.arange(xy.shape[0]), k)
    return np.stack([src, idx[:, 1:].reshape(-1)], 1)


def scene(n, k, share_unassigned, C, dtype, seed, cells=12):
    """Points in the unit square, a directed kNN graph, ``share_unassigned`` of them unassigned, and embeddings that agree
    inside a grid cell and disagree across cells: a basis vector per cell class plus noise, normalised -- the cosines are
    bimodal, far from 0.5 (asserted by the host test, not assumed).  -> (xy, Case of one batch)"""
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2))
    pairs = knn_pairs(xy, k)
    cell = (np.floor(xy[:, 0] * cells) * 7 + np.floor(xy[:, 1] * cells) * 3).astype(np.int64)
    z = 0.04 * rng.standard_normal((n, C))
    if C >= 3:
        z[np.arange(n), cell % min(C, 16)] += 1.0
    else:
        z[:, 0] += np.where(cell % 2 == 0, 1.0, -1.0)                 # C = 1, 2: the sign is the class
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    un = torch.as_tensor(rng.random(n) < share_unassigned)
    return xy, Case(n, un, [Batch(torch.tensor(z, dtype=torch.float32).to(dtype), edges(pairs))], 0.5, 5, 0)


def permuted(case: Case, seed=1) -> Case:
    b = case.batches[0]
    p = torch.as_tensor(np.random.default_rng(seed).permutation(b.edge_index.shape[1]))
    return case._replace(batches=[b._replace(edge_index=b.edge_index[:, p])])


def tiled(xy, case: Case, n_tiles=3, order=None) -> Case:
    """The one-batch scene as overlapping tiles with local ids: a tile owns a vertical strip (``mask``), holds the strip's
    points and every neighbour of one (so each directed edge is scored by exactly one tile) and every scene edge between
    two of its points -- those from a source it does not own are there to be masked out."""
    b = case.batches[0]
    s, d = b.edge_index.numpy()
    strip = np.minimum((xy[:, 0] * n_tiles).astype(np.int64), n_tiles - 1)
    batches = []
    for t in (range(n_tiles) if order is None else order):
        own = strip == t
        inside = own.copy()
        inside[d[own[s]]] = True
        nodes = np.nonzero(inside)[0]
        local = np.full(case.n, -1, np.int64)
        local[nodes] = np.arange(nodes.size)
        e = inside[s] & inside[d]
        ei = torch.tensor(np.stack([local[s[e]], local[d[e]]]))
        batches.append(Batch(b.z[torch.as_tensor(nodes)], ei, torch.as_tensor(nodes), torch.as_tensor(own[nodes])))
    return case._replace(batches=batches)


RANDOM = dict(n=20000, k=5, share_unassigned=0.4, C=64, dtype=torch.float32, seed=20)
WIDTHS = (1, 3, 64, 200)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def width_case(C, dtype):
    return scene(3000, 5, 0.5, C, dtype, seed=100 + C)[1]


def z_cases():
    """name -> Case for every seeded case of tests/test_gpu_fragments.py whose kept edges depend on a rounded cosine (the
    exact-threshold rows are small integers, for which every operation of the device cosine is exact: no margin is needed)"""
    out = {"random": scene(**RANDOM)[1]}
    xy, base = scene(**RANDOM)
    out["random_tiled"] = tiled(xy, base)
    for C in WIDTHS:
        for dt in DTYPES:
            out[f"width_{C}_{str(dt).split('.')[1]}"] = width_case(C, dt)
    for C, dt in ((8, torch.float32), (4, torch.float32), (24, torch.float16), (5, torch.bfloat16)):      # the structural cases' rows
        out[f"ones_{C}_{str(dt).split('.')[1]}"] = graph_case(4, [(0, 1), (2, 3)], C=C, dtype=dt)
    return out
