"""Phenograph clustering on the device: the reference's ``phenograph_rapids`` (``src/segger/data/utils/neighbors.py:18-51``:
cuML ``kneighbors`` -> cuGraph ``jaccard`` -> cuGraph ``louvain`` -> labels ranked by cluster size) without RAPIDS.

``knn_bruteforce`` is the hot path (``segger_knn_bruteforce``: fp32 MFMA inner products with the selection fused in);
``jaccard_graph`` builds the simple undirected graph of a neighbour table with torch's sort on the device and weighs it
with ``segger_jaccard_weights``; ``louvain`` is a deterministic, synchronous Louvain whose local moving and modularity
are ``segger_louvain_move`` / ``segger_louvain_modularity`` and whose aggregation is torch on the device;
``phenograph`` runs the three and relabels.  Device tensors in and out; there is no CPU path
(``tests/phenograph_cases.py`` holds the numpy restatement the tests compare against).

Louvain here, in full (the numpy oracle follows the same text):

* weights are 64-bit fixed point, ``round(w * 2**32)``: every sum of weights is an exact integer, whatever its order;
* a level starts from singletons; a round is ``SUBROUNDS`` sub-rounds, sub-round ``s`` moving the vertices with
  ``v % SUBROUNDS == s`` at once, each decided from the state at the start of the sub-round: the community of a
  neighbour with the largest ``g(c) = k_vc - (gamma * k_v) * tot_c / 2m`` (float64, this order of operations), the lowest
  id on a tie, only if it is strictly above ``g`` of staying, and never from a singleton into a singleton of a higher id;
* after each round ``Q`` is summed in a fixed order; the level ends when ``Q`` gained less than ``threshold`` (if it
  fell, the round is undone first), or after ``MAX_ROUNDS`` rounds;
* the modularity returned is that of the ORIGINAL float64 weights under the final labels (``_modularity_of``);
* communities are renumbered ``0..C-1`` in ascending id order, parallel edges summed, internal weight kept as a
  per-vertex self weight; the run ends when a level merged nothing, gained less than ``threshold``, or after
  ``max_level`` levels.

Not reproduced (cuML and cuGraph cannot be installed next to ROCm and were never run): cuGraph's treatment of the
``(i, i)`` pairs ``kneighbors`` returns -- they are dropped here, and only make the Jaccard neighbourhoods closed;
cuGraph's handling of duplicate pairs (the graph is made simple here); cuGraph's own, non-deterministic move order --
labels are comparable in quality (modularity), not cluster for cluster.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _lib as L

__all__ = ["knn_bruteforce", "jaccard_graph", "louvain", "phenograph", "relabel_by_size"]

SUBROUNDS = 4            # sub-rounds of a round: vertices v % SUBROUNDS == s move together
MAX_ROUNDS = 64          # rounds of a level, at most
FIXED_ONE = 1 << 32      # the fixed-point unit of Louvain's weights
_FIXED_LIMIT = float(1 << 61)


def knn_bruteforce(X: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """The exact ``k`` nearest rows of ``X`` ``[N, d]`` for every row of ``X``, itself included, as
    ``cuml.NearestNeighbors.kneighbors(X)`` on its own training set: ``idx`` ``[N, k]`` int32 and ``dist2`` ``[N, k]``
    float32 (squared Euclidean, recomputed directly), every row sorted by (dist2, idx).  ``X`` is cast to float32.
    ``1 <= d <= 256``, ``1 <= k <= min(64, N)``, else ``ValueError``.  Bit-identical from call to call."""
    L.need_device("knn_bruteforce", X)
    if X.dim() != 2:
        raise ValueError("knn_bruteforce: X is [N, d]")
    n, d, k = int(X.shape[0]), int(X.shape[1]), int(k)
    if not 1 <= d <= L.KNN_BF_MAX_D:
        raise ValueError(f"knn_bruteforce: d = {d} outside 1 .. {L.KNN_BF_MAX_D}")
    if not 1 <= k <= L.KNN_BF_MAX_K:
        raise ValueError(f"knn_bruteforce: k = {k} outside 1 .. {L.KNN_BF_MAX_K}")
    if k > n:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {n}")
    dev = X.device
    X = X.detach().to(torch.float32).contiguous()
    ws, ws_bytes = L.workspace("segger_knn_bruteforce_workspace_bytes", dev, n, d, k)
    idx = torch.empty(n, k, dtype=torch.int32, device=dev)
    dist2 = torch.empty(n, k, dtype=torch.float32, device=dev)
    L.call("segger_knn_bruteforce", dev, X.data_ptr(), n, d, k, idx.data_ptr(), dist2.data_ptr(), ws.data_ptr(), ws_bytes)
    return idx, dist2


def jaccard_graph(idx: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """The Jaccard graph of a neighbour table ``idx`` ``[N, k]``: drop ``i == j``, take the union of ``i -> j`` and
    ``j -> i``, deduplicate -- a simple undirected graph in CSR (``indptr`` int64 ``[N + 1]``, ``indices`` int32 ascending
    inside a row, both directions stored) -- and weigh every edge by ``|N[u] & N[v]| / |N[u] | N[v]|`` over the closed
    neighbourhoods (``weight`` float64, one division of two integers; the two directions of an edge carry the same bits)."""
    L.need_device("jaccard_graph", idx)
    if idx.dim() != 2:
        raise ValueError("jaccard_graph: idx is [N, k]")
    dev = idx.device
    n = int(idx.shape[0])
    src = torch.arange(n, dtype=torch.int64, device=dev).unsqueeze(1).expand_as(idx).reshape(-1)
    dst = idx.detach().reshape(-1).to(torch.int64)
    keep = (src != dst) & (dst >= 0) & (dst < n)
    src, dst = src[keep], dst[keep]
    key = torch.unique(torch.cat([src * n + dst, dst * n + src]))                  # sorted: row-major, columns ascending
    rows = torch.div(key, max(n, 1), rounding_mode="floor")
    indices = (key - rows * n).to(torch.int32)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    if n:
        torch.cumsum(torch.bincount(rows, minlength=n), 0, out=indptr[1:])
    nnz = int(indices.numel())
    weight = torch.empty(nnz, dtype=torch.float64, device=dev)
    L.call("segger_jaccard_weights", dev, indptr.data_ptr(), indices.data_ptr(), n, nnz, weight.data_ptr())
    return indptr, indices, weight


def _modularity(dev, indptr, indices, w, self_w, comm, tot, n, nnz, gamma, two_m, in_c, q) -> float:
    L.call("segger_louvain_modularity", dev, indptr.data_ptr(), indices.data_ptr(), w.data_ptr(), self_w.data_ptr(),
           comm.data_ptr(), tot.data_ptr(), n, nnz, gamma, two_m, in_c.data_ptr(), q.data_ptr())
    return float(q.item())                                                         # the one wait of a round


def louvain(indptr: Tensor, indices: Tensor, weight: Tensor, resolution: float = 1.0, max_level: int = 100,
            threshold: float = 1e-7, return_stats: bool = False):
    """Deterministic Louvain on a weighted undirected graph without self-loops (CSR, both directions stored): maximises
    ``Q = sum_c in_c / 2m - resolution * (tot_c / 2m)**2``.  Returns ``labels`` int32 ``[N]`` (``0..C-1``, in the
    ascending order of the last level's community ids) and ``modularity`` (float).  The same labels on every
    call.  ``return_stats`` adds a dict with the levels and rounds run.  The module docstring has the scheme."""
    L.need_device("louvain", indptr, indices, weight)
    dev = indptr.device
    lib = L.load()
    gamma = float(resolution)
    if gamma < 0:
        raise ValueError("louvain: resolution must not be negative")
    indptr = indptr.detach().to(torch.int64).contiguous().view(-1)
    indices = indices.detach().to(torch.int32).contiguous().view(-1)
    weight = weight.detach().to(torch.float64).contiguous().view(-1)
    n, nnz = int(indptr.numel()) - 1, int(indices.numel())
    if n < 0 or int(weight.numel()) != nnz:
        raise ValueError("louvain: indptr has N + 1 entries, indices and weight nnz")
    labels = torch.arange(n, dtype=torch.int64, device=dev)
    stats = {"levels": 0, "rounds": 0}
    total = float(weight.sum().item()) if nnz else 0.0
    if n == 0 or nnz == 0 or not total > 0.0:
        out = (labels.to(torch.int32), 0.0)
        return out + (stats,) if return_stats else out
    if not total * FIXED_ONE < _FIXED_LIMIT or bool((weight < 0).any()):
        raise ValueError("louvain: weights must be non-negative and sum to less than 2**29")
    w = torch.round(weight * float(FIXED_ONE)).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), indptr[1:] - indptr[:-1])
    rows0, cols0 = rows, indices.to(torch.int64)
    self_w = torch.zeros(n, dtype=torch.int64, device=dev)
    two_m = float(int(w.sum().item()))
    q_buf = torch.zeros(1, dtype=torch.float64, device=dev)
    q_final = 0.0
    for level in range(int(max_level)):
        kdeg = self_w.clone().index_add_(0, rows, w)
        comm = torch.arange(n, dtype=torch.int32, device=dev)
        tot = kdeg.clone()
        size = torch.ones(n, dtype=torch.int32, device=dev)
        proposal = torch.empty(n, dtype=torch.int32, device=dev)
        in_c = torch.empty(n, dtype=torch.int64, device=dev)
        args = (dev, indptr, indices, w, self_w)
        q_start = q_prev = _modularity(*args, comm, tot, n, nnz, gamma, two_m, in_c, q_buf)
        stats["levels"] += 1
        for _ in range(MAX_ROUNDS):
            comm_prev = comm.clone()
            with L.on_device(dev):                                                 # one guard around the four sub-rounds
                for sub in range(SUBROUNDS):
                    rc = lib.segger_louvain_move(indptr.data_ptr(), indices.data_ptr(), w.data_ptr(), kdeg.data_ptr(), n, nnz, sub,
                                                 SUBROUNDS, gamma, two_m, comm.data_ptr(), tot.data_ptr(), size.data_ptr(),
                                                 proposal.data_ptr(), L.stream_ptr(dev))
                    L.check(rc, "segger_louvain_move")
            stats["rounds"] += 1
            q_new = _modularity(*args, comm, tot, n, nnz, gamma, two_m, in_c, q_buf)
            if q_new < q_prev:                                                     # the round lost: undo it, the level is over
                comm = comm_prev
                break
            gain, q_prev = q_new - q_prev, q_new
            if gain < threshold:
                break
        q_final = q_prev
        unique, inverse = torch.unique(comm.to(torch.int64), sorted=True, return_inverse=True)
        n_new = int(unique.numel())
        if n_new == n:                                                             # nothing merged: the labels stand
            break
        labels = inverse[labels]
        cu, cv = inverse[rows], inverse[indices.to(torch.int64)]
        inner = cu == cv
        self_w = torch.zeros(n_new, dtype=torch.int64, device=dev).index_add_(0, inverse, self_w)
        self_w.index_add_(0, cu[inner], w[inner])
        key, pos = torch.unique(cu[~inner] * n_new + cv[~inner], sorted=True, return_inverse=True)
        w = torch.zeros(int(key.numel()), dtype=torch.int64, device=dev).index_add_(0, pos, w[~inner])
        rows = torch.div(key, n_new, rounding_mode="floor")
        indices = (key - rows * n_new).to(torch.int32)
        indptr = torch.zeros(n_new + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(rows, minlength=n_new), 0, out=indptr[1:])
        n, nnz = n_new, int(indices.numel())
        if q_prev - q_start < threshold or nnz == 0:
            break
    out = (labels.to(torch.int32), _modularity_of(weight, rows0, cols0, labels, gamma))
    return out + (stats,) if return_stats else out


def _modularity_of(weight: Tensor, rows: Tensor, cols: Tensor, labels: Tensor, gamma: float) -> float:
    """``Q`` of the ORIGINAL float64 weights under ``labels``: every weight is split into two 32-bit fixed-point parts
    (``hi = round(w 2^32)``, the part Louvain itself uses, and ``lo = round((w 2^32 - hi) 2^32)``), whose integer sums per
    cluster are exact in any order; the ``C`` terms are added on the host by numpy.  Bit-reproducible, and within a few
    float64 roundings of ``Q`` computed directly from the weights."""
    unique, inverse = torch.unique(labels, sorted=True, return_inverse=True)
    n_c = int(unique.numel())
    first = torch.full((n_c,), int(labels.numel()), dtype=torch.int64, device=labels.device).scatter_reduce_(
        0, inverse, torch.arange(int(labels.numel()), dtype=torch.int64, device=labels.device), reduce="amin")
    rank = torch.empty_like(first)
    rank[torch.argsort(first)] = torch.arange(n_c, dtype=torch.int64, device=labels.device)
    labels = rank[inverse]                                   # clusters numbered by their smallest vertex: one partition, one Q
    scaled = weight * float(FIXED_ONE)
    hi = torch.round(scaled)
    lo = torch.round((scaled - hi) * float(FIXED_ONE)).to(torch.int64)
    hi = hi.to(torch.int64)
    cu, inner = labels[rows], labels[rows] == labels[cols]
    sums = torch.zeros(4, n_c, dtype=torch.int64, device=weight.device)
    sums[0].index_add_(0, cu, hi)
    sums[1].index_add_(0, cu, lo)
    sums[2].index_add_(0, cu[inner], hi[inner])
    sums[3].index_add_(0, cu[inner], lo[inner])
    s = sums.cpu().numpy()
    two_m = (float(int(s[0].sum())) + float(int(s[1].sum())) / FIXED_ONE) / FIXED_ONE
    tot = (s[0].astype("float64") + s[1].astype("float64") / FIXED_ONE) / FIXED_ONE
    in_c = (s[2].astype("float64") + s[3].astype("float64") / FIXED_ONE) / FIXED_ONE
    x = tot / two_m
    return float((in_c / two_m - (gamma * x) * x).sum())


def relabel_by_size(labels: Tensor, min_size: int = -1) -> Tensor:
    """The reference's relabelling (``neighbors.py:45-51``): clusters ranked by size, descending -- on a tie the cluster
    holding the smallest vertex id first -- and a cluster with ``size > min_size`` gets its rank, the others -1.  The ranks
    are taken BEFORE the size filter, as the reference does.  int64."""
    labels = labels.to(torch.int64)
    n = int(labels.numel())
    if n == 0:
        return labels.clone()
    unique, inverse, counts = torch.unique(labels, sorted=True, return_inverse=True, return_counts=True)
    c = int(unique.numel())
    first = torch.full((c,), n, dtype=torch.int64, device=labels.device).scatter_reduce_(
        0, inverse, torch.arange(n, dtype=torch.int64, device=labels.device), reduce="amin")
    order = torch.argsort((n - counts) * (n + 1) + first)                          # size descending, then first vertex
    rank = torch.empty(c, dtype=torch.int64, device=labels.device)
    rank[order] = torch.arange(c, dtype=torch.int64, device=labels.device)
    rank = torch.where(counts > int(min_size), rank, torch.full_like(rank, -1))
    return rank[inverse]


def phenograph(X: Tensor, n_neighbors: int, resolution: float = 1.0, min_size: int = -1) -> Tensor:
    """``phenograph_rapids``: kNN of ``X`` (its float64 column means subtracted before the float32 cast -- distances do not
    change, the expanded form's cancellation shrinks), the Jaccard graph, Louvain at ``resolution``, labels ranked by
    cluster size with ``-1`` for clusters of ``min_size`` members or fewer.  int64 ``[N]``, on ``X``'s device."""
    L.need_device("phenograph", X)
    if X.dim() != 2:
        raise ValueError("phenograph: X is [N, d]")
    centred = X.detach().to(torch.float64)
    centred = (centred - centred.mean(dim=0, keepdim=True)) if centred.shape[0] else centred
    idx, _ = knn_bruteforce(centred.to(torch.float32), n_neighbors)
    labels, _ = louvain(*jaccard_graph(idx), resolution=resolution)
    return relabel_by_size(labels, min_size)
