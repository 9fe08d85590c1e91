"""Cases and numpy oracles of the phenograph clustering (``segger_amd.phenograph``, ``csrc/phenograph.hip``): the case
generators, a float64 kNN by direct distances ordered by (distance, index), the Jaccard graph by Python sets, and a
restatement of the SAME deterministic Louvain and relabelling the device runs (the scheme is written out in the
docstring of ``segger_amd/phenograph.py``; operation for operation the float64 expressions here are the kernels').
No GPU, no sklearn, no networkx: their numbers travel in tests/golden/phenograph_small.npz."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phenograph_small.npz")
SUBROUNDS, MAX_ROUNDS, FIXED_ONE, Q_THREADS = 4, 64, float(1 << 32), 256
U24 = 2.0 ** -24
REAL_K = 10
REAL_CASES = {"mix16": (16, 0.0), "mix128": (128, 0.0), "mix16_off": (16, 50.0)}        # name -> (d, mean)
QUALITY_CASES = ("planted300", "jaccard600_g1", "jaccard600_g2")


# ------------------------------------------------------------------ kNN ---
def lattice_case(n, d, seed, span=8, copies=0):
    """small integers: every product and sum of the expanded form is exact in fp32 (|x| <= 8, d <= 256), with many exact
    ties; ``copies`` rows at the END are made equal to row 0"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-span, span + 1, size=(n, d)).astype(np.float32)
    if copies:
        X[n - copies:] = X[0]
    return X


def mixture_case(n, d, mean, seed, n_types=8):
    rng = np.random.default_rng(seed)
    centres = 12.0 / np.sqrt(d) * rng.normal(size=(n_types, d))       # centre norms ~ 12 whatever d: tau stays small
    X = centres[rng.integers(0, n_types, n)] + rng.normal(size=(n, d))
    return (X - X.mean(axis=0) + mean).astype(np.float32)


def dist2_f64(X, rows=None):
    """[len(rows), N] squared distances, float64, directly as sum (a - b)^2"""
    X = np.asarray(X, dtype=np.float64)
    rows = np.arange(len(X)) if rows is None else rows
    out = np.empty((len(rows), len(X)))
    for s in range(0, len(rows), 64):
        out[s:s + 64] = ((X[rows[s:s + 64], None, :] - X[None, :, :]) ** 2).sum(axis=2)
    return out


def knn_oracle(X, k):
    D = dist2_f64(X)
    idx = np.argsort(D, axis=1, kind="stable")[:, :k]                 # stable: ties by index
    return idx.astype(np.int32), np.take_along_axis(D, idx, axis=1)


def knn_tau(X):
    """the fp32 expanded form's error bound per row: norms and the product are FMA chains of d terms, each within
    (d + 1) u of its exact value relative to |a|^2 + |b|^2 (Cauchy-Schwarz for the product, twice), plus the two final
    roundings: 4 (d + 3) 2^-24 (|x_i|^2 + max_j |x_j|^2)"""
    sq = (np.asarray(X, dtype=np.float64) ** 2).sum(axis=1)
    return 4.0 * (X.shape[1] + 3) * U24 * (sq + sq.max())


# ------------------------------------------------------------------ Jaccard ---
def jaccard_oracle(idx):
    n = len(idx)
    adj = [set() for _ in range(n)]
    for i in range(n):
        for j in idx[i]:
            j = int(j)
            if j != i:
                adj[i].add(j)
                adj[j].add(i)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indices, inter, union = [], [], []
    for u in range(n):
        nu = adj[u] | {u}
        for v in sorted(adj[u]):
            nv = adj[v] | {v}
            indices.append(v)
            inter.append(len(nu & nv))
            union.append(len(nu | nv))
        indptr[u + 1] = len(indices)
    weight = np.asarray(inter, dtype=np.float64) / np.asarray(union, dtype=np.float64)
    return indptr, np.asarray(indices, dtype=np.int32), weight.reshape(-1)


def csr_of_edges(n, edges, weights=None):
    """symmetric CSR (columns ascending, both directions) of undirected edges [(u, v)]"""
    w = np.ones(len(edges)) if weights is None else np.asarray(weights, dtype=np.float64)
    both = {}
    for (u, v), x in zip(edges, w):
        both[(u, v)] = x
        both[(v, u)] = x
    keys = sorted(both)
    indptr = np.zeros(n + 1, dtype=np.int64)
    for u, _ in keys:
        indptr[u + 1] += 1
    return (np.cumsum(indptr), np.asarray([v for _, v in keys], dtype=np.int32).reshape(-1),
            np.asarray([both[key] for key in keys], dtype=np.float64).reshape(-1))


def components(indptr, indices):
    n = len(indptr) - 1
    comp = np.full(n, -1, dtype=np.int64)
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s], stack = s, [s]
        while stack:
            u = stack.pop()
            for v in indices[indptr[u]:indptr[u + 1]]:
                if comp[v] < 0:
                    comp[v] = s
                    stack.append(int(v))
    return comp


# ------------------------------------------------------------------ Louvain ---
def _q_fixed_order(in_c, tot, gamma, two_m):
    x = tot.astype(np.float64) / two_m
    terms = in_c.astype(np.float64) / two_m - (gamma * x) * x
    pad = np.zeros(-(-len(terms) // Q_THREADS) * Q_THREADS)
    pad[:len(terms)] = terms
    acc = np.zeros(Q_THREADS)
    for row in pad.reshape(-1, Q_THREADS):                            # thread t: terms t, t + 256, ... in turn
        acc = acc + row
    s = Q_THREADS // 2
    while s:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return float(acc[0])


def _q_of(indptr, indices, rows, w, self_w, comm, tot, gamma, two_m):
    in_c = np.zeros(len(comm), dtype=np.int64)
    np.add.at(in_c, comm, self_w)
    inner = comm[rows] == comm[indices]
    np.add.at(in_c, comm[rows[inner]], w[inner])
    return _q_fixed_order(in_c, tot, gamma, two_m)


def louvain_oracle(indptr, indices, weight, resolution=1.0, max_level=100, threshold=1e-7):
    """-> labels int32, modularity, stats; the scheme of segger_amd/phenograph.py, vertex by vertex"""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    weight = np.asarray(weight, dtype=np.float64)
    n, gamma = len(indptr) - 1, float(resolution)
    labels = np.arange(n, dtype=np.int64)
    stats = {"levels": 0, "rounds": 0}
    if n == 0 or len(indices) == 0 or not weight.sum() > 0.0:
        return labels.astype(np.int32), 0.0, stats
    w = np.rint(weight * FIXED_ONE).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    rows0, cols0 = rows, indices
    self_w = np.zeros(n, dtype=np.int64)
    two_m = float(int(w.sum()))
    q_final = 0.0
    for _level in range(max_level):
        kdeg = self_w.copy()
        np.add.at(kdeg, rows, w)
        comm, tot, size = np.arange(n, dtype=np.int64), kdeg.copy(), np.ones(n, dtype=np.int64)
        q_start = q_prev = _q_of(indptr, indices, rows, w, self_w, comm, tot, gamma, two_m)
        stats["levels"] += 1
        for _round in range(MAX_ROUNDS):
            comm_prev = comm.copy()
            for sub in range(SUBROUNDS):
                c0, t0, s0 = comm.copy(), tot.copy(), size.copy()     # the state at the start of the sub-round
                for v in range(sub, n, SUBROUNDS):
                    nb, wv = indices[indptr[v]:indptr[v + 1]], w[indptr[v]:indptr[v + 1]]
                    cs, a, kv = c0[nb], int(c0[v]), int(kdeg[v])
                    gk = gamma * float(kv)
                    g_stay = float(int(wv[cs == a].sum())) - (gk * float(int(t0[a]) - kv)) / two_m
                    best_g, best_c = -np.inf, None
                    for c in np.unique(cs):                           # ascending: the lowest id wins a tie
                        c = int(c)
                        if c == a or (s0[a] == 1 and s0[c] == 1 and c > a):
                            continue
                        g = float(int(wv[cs == c].sum())) - (gk * float(int(t0[c]))) / two_m
                        if g > best_g:
                            best_g, best_c = g, c
                    if best_c is not None and best_g > g_stay:
                        comm[v] = best_c
                        tot[best_c] += kv
                        tot[a] -= kv
                        size[best_c] += 1
                        size[a] -= 1
            stats["rounds"] += 1
            q_new = _q_of(indptr, indices, rows, w, self_w, comm, tot, gamma, two_m)
            if q_new < q_prev:
                comm = comm_prev
                break
            gain, q_prev = q_new - q_prev, q_new
            if gain < threshold:
                break
        q_final = q_prev
        unique, inverse = np.unique(comm, return_inverse=True)
        inverse = inverse.reshape(-1)
        n_new = len(unique)
        if n_new == n:
            break
        labels = inverse[labels]
        cu, cv = inverse[rows], inverse[indices]
        inner = cu == cv
        new_self = np.zeros(n_new, dtype=np.int64)
        np.add.at(new_self, inverse, self_w)
        np.add.at(new_self, cu[inner], w[inner])
        key, pos = np.unique(cu[~inner] * n_new + cv[~inner], return_inverse=True)
        new_w = np.zeros(len(key), dtype=np.int64)
        np.add.at(new_w, pos.reshape(-1), w[~inner])
        self_w, w, rows, indices = new_self, new_w, key // n_new, key % n_new
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_new))]).astype(np.int64)
        n = n_new
        if q_prev - q_start < threshold or len(indices) == 0:
            break
    return labels.astype(np.int32), modularity_exact(weight, rows0, cols0, labels, gamma), stats


def modularity_exact(weight, rows, cols, labels, gamma):
    """Q of the original float64 weights from exact hi / lo fixed-point sums, as ``segger_amd.phenograph._modularity_of``"""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))                   # clusters numbered by their smallest vertex: the
    labels = rank[inverse.reshape(-1)]                                # same partition gives the same bits
    n_c = len(first)
    scaled = weight * FIXED_ONE
    hi = np.rint(scaled)
    lo = np.rint((scaled - hi) * FIXED_ONE).astype(np.int64)
    hi = hi.astype(np.int64)
    cu, inner = labels[rows], labels[rows] == labels[cols]
    s = np.zeros((4, n_c), dtype=np.int64)
    np.add.at(s[0], cu, hi)
    np.add.at(s[1], cu, lo)
    np.add.at(s[2], cu[inner], hi[inner])
    np.add.at(s[3], cu[inner], lo[inner])
    two_m = (float(int(s[0].sum())) + float(int(s[1].sum())) / FIXED_ONE) / FIXED_ONE
    tot = (s[0].astype(np.float64) + s[1].astype(np.float64) / FIXED_ONE) / FIXED_ONE
    in_c = (s[2].astype(np.float64) + s[3].astype(np.float64) / FIXED_ONE) / FIXED_ONE
    x = tot / two_m
    return float((in_c / two_m - (gamma * x) * x).sum())


def modularity_f64(indptr, indices, weight, labels, resolution=1.0):
    """Q straight from its definition in float64 (independent of the fixed-point path)"""
    indptr, labels = np.asarray(indptr), np.asarray(labels)
    weight = np.asarray(weight, dtype=np.float64)
    two_m = weight.sum()
    if not two_m > 0:
        return 0.0
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    c = labels.max() + 1
    tot = np.bincount(labels[rows], weights=weight, minlength=c)
    inner = labels[rows] == labels[np.asarray(indices)]
    in_c = np.bincount(labels[rows[inner]], weights=weight[inner], minlength=c)
    return float((in_c / two_m - resolution * (tot / two_m) ** 2).sum())


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(a) == len(b) and len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def relabel_oracle(labels, min_size=-1):
    """neighbors.py:45-51: ranks by size (descending; ties: the cluster holding the smallest vertex first), taken BEFORE
    the size filter, then -1 for size <= min_size"""
    labels = np.asarray(labels)
    first, count = {}, {}
    for v, c in enumerate(labels.tolist()):
        first.setdefault(c, v)
        count[c] = count.get(c, 0) + 1
    order = sorted(count, key=lambda c: (-count[c], first[c]))
    rank = {c: (r if count[c] > min_size else -1) for r, c in enumerate(order)}
    return np.asarray([rank[c] for c in labels.tolist()], dtype=np.int64)


def ring_of_cliques(n_cliques=8, size=6):
    edges = []
    for q in range(n_cliques):
        base = q * size
        edges += [(base + i, base + j) for i in range(size) for j in range(i + 1, size)]
        edges.append((base + size - 1, ((q + 1) % n_cliques) * size))
    return csr_of_edges(n_cliques * size, edges)


def planted_partition(n=300, groups=6, p_in=0.25, p_out=0.01, seed=5):
    rng = np.random.default_rng(seed)
    block = rng.integers(0, groups, n)
    edges, weights = [], []
    for u in range(n):
        for v in range(u + 1, n):
            if rng.random() < (p_in if block[u] == block[v] else p_out):
                edges.append((u, v))
                weights.append(0.25 + 1.75 * rng.random())
    return csr_of_edges(n, edges, weights)


def jaccard600():
    X = mixture_case(600, 8, 0.0, seed=23, n_types=6)
    return jaccard_oracle(knn_oracle(X, 10)[0])


def louvain_cases():
    """name -> (indptr, indices, weight, resolution)"""
    k88 = csr_of_edges(16, [(u, 8 + v) for u in range(8) for v in range(8)])
    triangles = csr_of_edges(6, [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)])
    edgeless = (np.zeros(8, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    j600 = jaccard600()
    return {"ring": ring_of_cliques() + (1.0,), "triangles": triangles + (1.0,), "edge": csr_of_edges(2, [(0, 1)]) + (1.0,),
            "edgeless": edgeless + (1.0,), "planted300": planted_partition() + (1.0,), "jaccard600_g1": j600 + (1.0,),
            "jaccard600_g2": j600 + (2.0,), "k88": k88 + (1.0,)}
