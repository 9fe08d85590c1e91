#!/usr/bin/env python
"""Time the boundary and gene features on the GPU: ``features.expression_features`` (csrc/features.hip: a float64 MFMA
Gram of the sparse rows and a CSR x dense projection) against the torch formulation that was available before it -- CSR ->
dense float64 -> ``torch.corrcoef`` / ``torch.cov`` -> the same ``eigh`` -> dense matmul -- on the same synthetic count
matrix, already on the device.

Per size (``--cells``, default 10^5 and 10^6): ``cells`` cells x 500 genes, about 60 counts per cell drawn from a skewed
gene distribution mixed from 8 cell types, as canonical CSR with the dtypes ``expression_matrix`` returns.  The two paths
are run alternately ``--runs`` times after one warm-up each at that size and the medians are reported:

* seconds: a host clock around work that ends in a device synchronise;
* peak bytes: ``torch.cuda.max_memory_allocated`` over the phase minus what was allocated when it began (the inputs);
* the two kernels on their own (``sparse_gram``, ``sparse_project`` at k = 128, float32 out) and the rate of the Gram in
  float64 FLOP/s of the dense product it performs (2 x 64 x 64 per row, per tile pair);
* how far the two paths are apart: ``corr`` and ``X_pca`` (largest absolute difference; the components of synthetic
  counts are close together, so ``X_pca`` is also compared through the explained variances).

One JSON line; ``--out`` also writes it to a file (profiles/features_cells_per_s.json is the committed measurement)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_GENES = 500
N_TYPES = 8
DEPTH = 60


def make_cells(n_cells: int, device, seed: int):
    """-> the dict ``expression_matrix`` returns (the CSR part of it) for ``n_cells`` synthetic cells"""
    g = torch.Generator(device=device).manual_seed(seed)
    profile = torch.softmax(1.5 * torch.randn(N_TYPES, N_GENES, generator=g, device=device), dim=1)
    kind = torch.randint(0, N_TYPES, (n_cells,), generator=g, device=device)
    depth = torch.randint(DEPTH // 3, 2 * DEPTH - DEPTH // 3 + 1, (n_cells,), generator=g, device=device)
    depth[torch.rand(n_cells, generator=g, device=device) < 0.02] = 4                     # cells below cells_min_counts
    keys = []
    for t in range(N_TYPES):                                                              # one multinomial per cell type
        cells = (kind == t).nonzero().squeeze(1)
        draws = torch.multinomial(profile[t], int(cells.numel()) * 2 * DEPTH, replacement=True, generator=g)
        draws = draws.view(-1, 2 * DEPTH)
        used = torch.arange(2 * DEPTH, device=device)[None, :] < depth[cells][:, None]
        keys.append((cells[:, None] * N_GENES + draws)[used])
    pair, counts = torch.unique(torch.cat(keys), return_counts=True)                       # sorted: canonical CSR
    row = pair // N_GENES
    indptr = torch.zeros(n_cells + 1, dtype=torch.int64, device=device)
    indptr[1:] = torch.bincount(row, minlength=n_cells).cumsum(0)
    return {"indptr": indptr, "indices": (pair % N_GENES).int(), "counts": counts.int(),
            "gene_ids": torch.arange(N_GENES, dtype=torch.int32, device=device)}


def torch_features(expr, k: int, cells_min_counts: int, genes_min_counts: int, out_dtype=torch.float32):
    """the same numbers from a dense float64 matrix: what torch alone offers"""
    from segger_amd.features import _top_eigenvectors
    indptr, indices, counts = expr["indptr"], expr["indices"], expr["counts"]
    n, dev = int(indptr.numel()) - 1, indptr.device
    rows = torch.repeat_interleave(torch.arange(n, device=dev), indptr.diff(), output_size=int(indices.numel()))
    dense = torch.zeros(n, int(expr["gene_ids"].numel()), dtype=torch.float64, device=dev)
    dense[rows, indices.long()] = counts.double()
    gene_keep = dense.sum(dim=0) >= genes_min_counts
    dense = dense[:, gene_keep]
    n_counts = dense.sum(dim=1)
    filtered = n_counts >= cells_min_counts
    ordered = n_counts[filtered].sort().values
    m = int(ordered.numel())
    target_sum = (ordered[(m - 1) // 2] + ordered[m // 2]) / 2.0
    dense *= torch.where(n_counts > 0, target_sum / n_counts, torch.zeros_like(n_counts))[:, None]
    fit = dense[filtered]
    corr = torch.nan_to_num(torch.corrcoef(fit.T), nan=0.0, posinf=1.0, neginf=1.0)
    centred = corr - corr.mean(dim=0, keepdim=True)
    X_corr = centred @ _top_eigenvectors(centred.T @ centred, k)[1]
    ev, V = _top_eigenvectors(torch.cov(fit.T), k)
    mean = fit.mean(dim=0)
    del fit
    X_pca = (dense @ V - mean @ V).to(out_dtype)
    return {"X_pca": X_pca, "X_corr": X_corr, "corr": corr, "gene_keep": gene_keep, "n_counts": n_counts.long(),
            "filtered": filtered, "target_sum": target_sum, "explained_variance": ev}


def phase(fn):
    """-> (result, seconds, peak bytes above what was allocated at the start)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return out, dt, torch.cuda.max_memory_allocated() - base


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", default="100000,1000000", help="cell counts, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--embedding-size", type=int, default=128)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_features.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import _lib
    from segger_amd.features import expression_features, sparse_gram, sparse_project

    dev = torch.device("cuda:0")
    k = args.embedding_size
    sizes = []
    for n in [int(s) for s in args.cells.split(",") if s]:
        expr = make_cells(n, dev, args.seed)
        torch.cuda.empty_cache()
        entry = {"cells": n, "n_genes": N_GENES, "nnz": int(expr["indices"].numel()), "embedding_size": k,
                 "input_bytes": torch.cuda.memory_allocated()}
        weight = torch.rand(n, dtype=torch.float64, device=dev) + 0.5
        V = torch.randn(N_GENES, k, dtype=torch.float64, device=dev)
        offset = torch.randn(k, dtype=torch.float64, device=dev)
        runs = {"hip": [], "torch": [], "gram": [], "project": []}
        for r in range(args.runs + 1):                               # run 0 warms every path up at this size
            got, t_a, p_a = phase(lambda: expression_features(expr, k))
            ref, t_b, p_b = phase(lambda: torch_features(expr, k, 10, 100))
            _, t_g, p_g = phase(lambda: sparse_gram(expr["indptr"], expr["indices"], expr["counts"], weight, N_GENES))
            _, t_p, p_p = phase(lambda: sparse_project(expr["indptr"], expr["indices"], expr["counts"], weight, V, offset))
            if r == 0:
                entry["n_filtered"] = int(got["filtered"].sum())
                entry["n_genes_kept"] = int(got["gene_keep"].sum())
                entry["integers_equal"] = all(torch.equal(got[key], ref[key]) for key in ("gene_keep", "n_counts", "filtered"))
                entry["corr_max_abs_diff"] = float((got["corr"] - ref["corr"]).abs().max())
                entry["X_pca_max_abs_diff"] = float((got["X_pca"].double() - ref["X_pca"].double()).abs().max())
                entry["X_pca_max_abs"] = float(ref["X_pca"].abs().max())
                entry["explained_variance_max_rel_diff"] = float(((got["explained_variance"] - ref["explained_variance"]).abs()
                                                                  / ref["explained_variance"][0]).max())
            else:
                for name, t, p in (("hip", t_a, p_a), ("torch", t_b, p_b), ("gram", t_g, p_g), ("project", t_p, p_p)):
                    runs[name].append((t, p))
            del got, ref
        for name, rs in runs.items():
            sec = statistics.median(t for t, _ in rs)
            entry[name] = {"seconds_median": sec, "seconds": [t for t, _ in rs], "cells_per_s": n / sec,
                           "peak_bytes_above_inputs": max(p for _, p in rs)}
        tiles = -(-N_GENES // _lib.FEATURES_TILE)
        flop = 2.0 * n * (tiles * (tiles + 1) // 2) * _lib.FEATURES_TILE ** 2
        entry["gram"]["dense_flop"] = flop
        entry["gram"]["dense_flop_per_s"] = flop / entry["gram"]["seconds_median"]
        entry["gram"]["slabs"] = int(_lib.load().segger_features_gram_slabs(n, N_GENES))
        entry["seconds_ratio_torch_over_hip"] = entry["torch"]["seconds_median"] / entry["hip"]["seconds_median"]
        entry["peak_ratio_torch_over_hip"] = (entry["torch"]["peak_bytes_above_inputs"]
                                              / max(entry["hip"]["peak_bytes_above_inputs"], 1))
        sizes.append(entry)
        print(f"[features] {entry}", file=sys.stderr, flush=True)
        del expr, weight, V, offset
        torch.cuda.empty_cache()
    res = {"what": "expression_features (HIP Gram + projection) vs dense float64 corrcoef / cov / matmul (torch) on synthetic cells",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "host clock around work ending in a device synchronise; median of the runs after one warm-up; "
                     "the paths alternate", "sizes": sizes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
