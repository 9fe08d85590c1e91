#!/usr/bin/env python
"""Time the contamination scoring on the GPU: ``validation.calculate_contamination`` (csrc/contamination.hip: the neighbour
frequencies and the three-way posterior of every stored count) against the reference's arithmetic restated in device
torch -- ``neigh[rows]``, ``L[:, gene_idx].T``, their float32 product and row sum, as ``contamination.py`` writes them --
chunked over the stored entries so that its ``chunk x T`` intermediates fit.

Per size (``--cells``, default 10^5 and 10^6): synthetic cells on a jittered lattice with about 50 stored genes each out of
``G = 500``, ``T = 32`` types, a random ``pc * me`` table, as canonical CSR with the dtypes ``expression_matrix`` returns.
The paths are run alternately ``--runs`` times (default 20) after one warm-up each and the medians are reported:

* seconds: a host clock around work that ends in a device synchronise;
* peak bytes: ``torch.cuda.max_memory_allocated`` over the phase minus what was allocated when it began (the inputs);
* the two kernels (``segger_neighbor_frequencies`` on a precomputed neighbour table, ``segger_contamination_posterior`` on
  prepared tensors): device events around one call of the thin wrapper whose only launch is the kernel, so the figure
  still holds that wrapper's host time where the kernel is shorter than it; for the posterior its compulsory bytes per
  stored entry (8 read, 16 written, plus the row's share of indptr, type, frequencies and the three per-row outputs)
  against that time as a share of 8 TB/s;
* ``--lds-genes`` (default 400): the posterior kernel once more at the largest size with a table that fits the kernel's
  LDS budget (``G = 500`` at ``T = 32`` does not and goes through L2), so that both table routes are timed;
* how far the two paths are apart (largest absolute difference of ``q_self``; the torch path sums in float32).

One JSON line; ``--out`` also writes it to a file (profiles/contamination_cells_per_s.json is the committed measurement).
A size that fails (for instance for lack of memory) is recorded with its error instead of being dropped."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_GENES = 500
N_TYPES = 32
DEPTH = 50
HBM_BYTES_PER_S = 8e12


def make_cells(n_cells: int, device, seed: int, n_genes: int = N_GENES):
    """-> (expr dict as ``expression_matrix(..., xy=)`` returns it, cell types, the [T, G] weight table)"""
    g = torch.Generator(device=device).manual_seed(seed)
    side = int(n_cells ** 0.5) + 1
    ids = torch.arange(n_cells, device=device)
    xy = torch.stack([ids % side, ids // side], 1).double() * 10.0 + 6.0 * torch.rand(n_cells, 2, generator=g, device=device).double()
    kind = torch.randint(0, N_TYPES, (n_cells,), generator=g, device=device, dtype=torch.int32)
    kind[torch.rand(n_cells, generator=g, device=device) < 0.02] = -1
    genes = torch.randint(0, n_genes, (n_cells, DEPTH + 3), generator=g, device=device)
    pair = torch.unique((ids[:, None] * n_genes + genes).view(-1))                        # sorted: canonical CSR
    indptr = torch.zeros(n_cells + 1, dtype=torch.int64, device=device)
    indptr[1:] = torch.bincount(pair // n_genes, minlength=n_cells).cumsum(0)
    counts = torch.randint(1, 9, (int(pair.numel()),), generator=g, device=device, dtype=torch.int32)
    weight = torch.rand(N_TYPES, n_genes, generator=g, device=device).double() * \
        (torch.rand(N_TYPES, n_genes, generator=g, device=device) < 0.6)
    expr = {"indptr": indptr, "indices": (pair % n_genes).int(), "counts": counts,
            "gene_ids": torch.arange(n_genes, dtype=torch.int32, device=device), "centroid": xy}
    return expr, kind, weight


def torch_contamination(expr, kind, weight, freq, chunk: int, alpha=(0.8, 0.15, 0.05), eps=1e-6, cutoff=0.5):
    """the reference's ``calculate_contamination`` after the frequencies, in device torch, ``chunk`` entries at a time"""
    indptr, indices, counts = expr["indptr"], expr["indices"], expr["counts"]
    dev, n, nnz = indptr.device, int(indptr.numel()) - 1, int(indices.numel())
    lik = weight.float() + eps
    labelled = kind[kind >= 0].long()
    back = (torch.bincount(labelled, minlength=lik.shape[0]).double() / max(int(labelled.numel()), 1)) @ lik.double()
    rows = torch.repeat_interleave(torch.arange(n, device=dev), indptr.diff(), output_size=nnz)
    q = torch.empty(3, nnz, dtype=torch.float32, device=dev)
    flagged = torch.empty(nnz, dtype=torch.int32, device=dev)
    for lo in range(0, nnz, chunk):
        r, g = rows[lo:lo + chunk], indices[lo:lo + chunk].long()
        host = kind[r].long()
        has = host >= 0
        p_self = torch.where(has, lik[host.clamp_min(0), g].double(), torch.full((), eps, dtype=torch.float64, device=dev))
        nv = freq[r]                                                                     # chunk x T, the reference's neigh[rows]
        nv[has.nonzero().squeeze(1), host[has]] = 0.0
        p_neigh = (nv * lik[:, g].T).sum(dim=1).double() + eps                           # two more chunk x T matrices
        p_back = back[g] + eps
        qs, qn, qb = alpha[0] * p_self, alpha[1] * p_neigh, alpha[2] * p_back
        denom = qs + qn + qb
        q[0, lo:lo + chunk], q[1, lo:lo + chunk], q[2, lo:lo + chunk] = qs / denom, qn / denom, qb / denom
        flagged[lo:lo + chunk] = torch.where(qs / denom < cutoff, counts[lo:lo + chunk], torch.zeros_like(counts[lo:lo + chunk]))
    contaminated = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, rows, flagged.long())
    total = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, rows, counts.long())
    return {"q_self": q[0], "q_neighbor": q[1], "q_background": q[2], "contamination": flagged, "contaminated": contaminated,
            "total": total, "percent_contamination": 100.0 * contaminated.double() / total.clamp_min(1).double()}


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


def device_ms(fn):
    """milliseconds between two device events around ``fn``"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def posterior_inputs(expr, kind, weight, freq):
    from segger_amd import validation as va
    lik_t, back = va._likelihood(weight, kind, int(weight.shape[0]), 1e-6)
    return (expr["indptr"], expr["indices"], expr["counts"], expr["gene_ids"], kind, freq, lik_t, back, int(weight.shape[0]))


def posterior_kernel_entry(n, nnz, n_types, ms):
    sec = statistics.median(ms) / 1e3
    moved = nnz * 24 + n * (8 + 4 + 4 * n_types + 24)
    return {"seconds_median": sec, "seconds": [m / 1e3 for m in ms], "cells_per_s": n / sec,
            "how": "device events around validation.contamination_posterior on prepared tensors (one launch)",
            "bytes_per_stored_entry": moved / nnz, "bytes_per_s": moved / sec, "share_of_8_TB_per_s": moved / sec / HBM_BYTES_PER_S}


def table_in_lds(n_types: int, n_genes: int) -> bool:
    """the rule of csrc/contamination.hip (include/segger_amd.h): padded table + four strips within SEGGER_CONTAM_LDS_BYTES"""
    from segger_amd import _lib
    tp = (n_types + 3) // 4 * 4
    ld_s = tp if (tp // 4) % 2 else tp + 4
    return (n_genes * ld_s + 4 * tp) * 4 <= _lib.CONTAM_LDS_BYTES


def measure(n: int, args, dev):
    from segger_amd import validation as va
    from segger_amd.neighbors import knn_grid
    expr, kind, weight = make_cells(n, dev, args.seed)
    torch.cuda.empty_cache()
    nnz = int(expr["indices"].numel())
    entry = {"cells": n, "n_genes": N_GENES, "n_types": N_TYPES, "nnz": nnz, "n_neighbors": args.k,
             "table_in_lds": table_in_lds(N_TYPES, N_GENES), "input_bytes": torch.cuda.memory_allocated(),
             "torch_chunk_entries": args.chunk}
    knn = knn_grid(expr["centroid"], args.k, return_dist=True)
    freq, _ = va.neighbor_frequencies(expr["centroid"], kind, args.k, N_TYPES, 20.0, knn=knn)
    prepared = posterior_inputs(expr, kind, weight, freq)
    runs = {"hip": [], "torch": []}
    freq_ms, post_ms = [], []
    for r in range(args.runs + 1):                                   # run 0 warms every path up at this size
        got, t_a, p_a = phase(lambda: va.calculate_contamination(expr, kind, weight))
        ref, t_b, p_b = phase(lambda: torch_contamination(expr, kind, weight, freq, args.chunk))
        m_f = device_ms(lambda: va.neighbor_frequencies(expr["centroid"], kind, args.k, N_TYPES, 20.0, knn=knn))
        m_p = device_ms(lambda: va.contamination_posterior(*prepared))
        if r == 0:
            entry["integers_equal"] = all(torch.equal(got[key], ref[key]) for key in ("total", "contaminated", "contamination"))
            entry["flags_differing"] = int((got["contamination"] != ref["contamination"]).sum())
            entry["q_self_max_abs_diff"] = float((got["q_self"].double() - ref["q_self"].double()).abs().max())
            entry["mean_percent_contamination"] = float(got["percent_contamination"].mean())
        else:
            runs["hip"].append((t_a, p_a))
            runs["torch"].append((t_b, p_b))
            freq_ms.append(m_f)
            post_ms.append(m_p)
        del got, ref
    for name, rs in runs.items():
        sec = statistics.median(t for t, _ in rs)
        entry[name] = {"seconds_median": sec, "seconds": [t for t, _ in rs], "cells_per_s": n / sec,
                       "peak_bytes_above_inputs": max(p for _, p in rs)}
    sec = statistics.median(freq_ms) / 1e3
    entry["frequencies_kernel"] = {"seconds_median": sec, "seconds": [m / 1e3 for m in freq_ms], "cells_per_s": n / sec,
                                   "how": "device events around validation.neighbor_frequencies(knn=...) (one launch)"}
    entry["posterior_kernel"] = posterior_kernel_entry(n, nnz, N_TYPES, post_ms)
    entry["seconds_ratio_torch_over_posterior_kernel"] = entry["torch"]["seconds_median"] / entry["posterior_kernel"]["seconds_median"]
    entry["nnz_x_T_float32_bytes_never_built"] = nnz * N_TYPES * 4
    return entry


def measure_lds_route(n: int, args, dev):
    """the posterior kernel alone with ``--lds-genes`` genes: the table-in-LDS route at the same T and cells"""
    from segger_amd import validation as va
    from segger_amd.neighbors import knn_grid
    expr, kind, weight = make_cells(n, dev, args.seed, args.lds_genes)
    nnz = int(expr["indices"].numel())
    knn = knn_grid(expr["centroid"], args.k, return_dist=True)
    freq, _ = va.neighbor_frequencies(expr["centroid"], kind, args.k, N_TYPES, 20.0, knn=knn)
    prepared = posterior_inputs(expr, kind, weight, freq)
    ms = [device_ms(lambda: va.contamination_posterior(*prepared)) for _ in range(args.runs + 1)][1:]
    entry = {"cells": n, "n_genes": args.lds_genes, "n_types": N_TYPES, "nnz": nnz, "table_in_lds": table_in_lds(N_TYPES, args.lds_genes),
             "posterior_kernel": posterior_kernel_entry(n, nnz, N_TYPES, ms)}
    return entry


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", default="100000,1000000", help="cell counts, comma separated")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=1 << 22, help="stored entries per chunk of the torch path")
    ap.add_argument("--lds-genes", type=int, default=400, help="gene count of the extra table-in-LDS timing (0: skip)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contamination.py needs an MI355X: a CPU timing says nothing about it")
    dev = torch.device("cuda:0")
    sizes, cells = [], [int(s) for s in args.cells.split(",") if s]
    jobs = [(n, measure) for n in cells] + ([(max(cells), measure_lds_route)] if args.lds_genes > 0 and cells else [])
    lds_route = None
    for n, job in jobs:
        try:
            entry = job(n, args, dev)
        except (RuntimeError, MemoryError) as e:                     # recorded, not hidden: the file says which size is missing
            entry = {"cells": n, "not_measured": f"{type(e).__name__}: {str(e)[:300]}"}
        if job is measure:
            sizes.append(entry)
        else:
            lds_route = entry
        print(f"[contamination] {entry}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    res = {"what": "calculate_contamination (HIP frequencies + posterior) vs the reference's nnz x T arithmetic in device torch, "
                   "chunked, on synthetic cells",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "host clock around work ending in a device synchronise; median of the runs after one warm-up; "
                     "the paths alternate; the torch path starts from precomputed frequencies, the hip path includes the "
                     "neighbour search and the frequency kernel; the two kernel figures are device events around one "
                     "call of a one-launch wrapper", "sizes": sizes, "posterior_table_in_lds": lds_route}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
