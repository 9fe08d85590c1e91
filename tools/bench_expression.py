#!/usr/bin/env python
"""Time the expression matrix on the GPU: ``postprocess.expression_matrix`` (csrc/expression.hip) against the torch
formulation of the same group-by (a sort of the pair keys, ``unique_consecutive``, ``index_add_``) on the same synthetic
deduplicated columns, already on the device.

Per size (``--rows``, default 10^6 and 10^7): ``rows`` transcripts over ``rows / 100`` cells and 500 genes, a tenth
unassigned, per-gene thresholds that keep about two thirds of the rest, positions for the centroids.  The two paths are
run alternately ``--runs`` times after one warm-up each at that size and the medians are reported:

* seconds: a host clock around work that ends in a device synchronise;
* peak bytes: ``torch.cuda.max_memory_allocated`` over the phase minus what was allocated when it began (the inputs);
* whether counts, ids and row pointers are equal, and the largest difference of the means and centroids -- the torch
  path sums with floating-point atomics (``index_add_``), so its float64 sums are not reproducible from run to run.

One JSON line; ``--out`` also writes it to a file (profiles/expression_rows_per_s.json is the committed measurement)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_GENES = 500


def make_columns(n: int, device, seed: int):
    g = torch.Generator(device=device).manual_seed(seed)
    n_cells = max(n // 100, 1)
    cell = torch.randint(0, n_cells, (n,), generator=g, device=device)
    cell = torch.where(torch.rand(n, generator=g, device=device) < 0.1, torch.full_like(cell, -1), cell)
    gene = torch.randint(0, N_GENES, (n,), generator=g, device=device)
    sim = torch.rand(n, generator=g, device=device) * 2 - 1
    gene_thr = (torch.rand(N_GENES, generator=g, device=device) * 0.6 - 0.6).double()
    xy = torch.rand(n, 2, generator=g, device=device) * 20000.0
    result = {"row_index": torch.arange(n, device=device), "cell_encoding": cell, "gene": gene, "similarity": sim,
              "similarity_threshold": gene_thr[gene]}
    return result, xy, n_cells


def torch_expression(result, xy, n_cells: int, n_genes: int):
    """The same outputs with torch ops only: filter, sort of the pair keys, unique_consecutive, index_add_."""
    keep = (result["cell_encoding"] >= 0) & (result["similarity"].double() >= result["similarity_threshold"])
    cell, gene = result["cell_encoding"][keep], result["gene"][keep]
    sim, pts = result["similarity"][keep].double(), xy[result["row_index"][keep]].double()
    key, order = torch.sort(cell * n_genes + gene, stable=True)
    pair, inv, counts = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    sums = torch.zeros(pair.numel(), dtype=torch.float64, device=key.device).index_add_(0, inv, sim[order])
    pc, pg = pair // n_genes, pair % n_genes
    cell_ids, row, n_pairs = torch.unique_consecutive(pc, return_inverse=True, return_counts=True)
    gene_ids, col = torch.unique(pg, return_inverse=True)
    indptr = torch.cat([n_pairs.new_zeros(1), n_pairs.cumsum(0)])
    cell_count = torch.zeros(cell_ids.numel(), dtype=torch.int64, device=key.device).index_add_(0, row, counts)
    cpos = row[inv]
    centroid = torch.zeros(cell_ids.numel(), 2, dtype=torch.float64, device=key.device).index_add_(0, cpos, pts[order])
    return {"cell_ids": cell_ids.int(), "gene_ids": gene_ids.int(), "indptr": indptr, "indices": col.int(),
            "counts": counts.int(), "mean_similarity": sums / counts, "cell_count": cell_count,
            "centroid": centroid / cell_count[:, None]}


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
    ap.add_argument("--rows", default="1000000,10000000", help="row counts, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_expression.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd.postprocess import expression_matrix

    dev = torch.device("cuda:0")
    sizes = []
    for n in [int(s) for s in args.rows.split(",") if s]:
        result, xy, n_cells = make_columns(n, dev, args.seed)
        torch.cuda.empty_cache()
        input_bytes = torch.cuda.memory_allocated()
        runs = {"hip": [], "torch": []}
        entry = {"rows": n, "n_cells": n_cells, "n_genes": N_GENES, "input_bytes": input_bytes}
        for r in range(args.runs + 1):                               # run 0 warms both paths up at this size
            got, t_a, p_a = phase(lambda: expression_matrix(result, xy, n_cells=n_cells, n_genes=N_GENES))
            ref, t_b, p_b = phase(lambda: torch_expression(result, xy, n_cells, N_GENES))
            if r == 0:
                entry["nnz"] = int(got["counts"].numel())
                entry["n_kept"] = int(got["n_kept"])
                entry["integers_equal"] = all(torch.equal(got[k], ref[k]) for k in
                                              ("cell_ids", "gene_ids", "indptr", "indices", "counts", "cell_count"))
                entry["mean_similarity_max_abs_diff"] = float((got["mean_similarity"] - ref["mean_similarity"]).abs().max())
                entry["centroid_max_abs_diff"] = float((got["centroid"] - ref["centroid"]).abs().max())
            else:
                runs["hip"].append((t_a, p_a))
                runs["torch"].append((t_b, p_b))
            del got, ref
        for name, rs in runs.items():
            sec = statistics.median(t for t, _ in rs)
            entry[name] = {"seconds_median": sec, "seconds": [t for t, _ in rs], "rows_per_s": n / sec,
                           "peak_bytes_above_inputs": max(p for _, p in rs)}
        entry["seconds_ratio_torch_over_hip"] = entry["torch"]["seconds_median"] / entry["hip"]["seconds_median"]
        entry["peak_ratio_torch_over_hip"] = (entry["torch"]["peak_bytes_above_inputs"]
                                              / max(entry["hip"]["peak_bytes_above_inputs"], 1))
        sizes.append(entry)
        print(f"[expression] {entry}", file=sys.stderr, flush=True)
        del result, xy
        torch.cuda.empty_cache()
    res = {"what": "expression_matrix (HIP) vs sort + unique_consecutive + index_add_ (torch) on synthetic rows",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "host clock around work ending in a device synchronise; median of the runs after one warm-up; "
                     "the two paths alternate", "sizes": sizes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
