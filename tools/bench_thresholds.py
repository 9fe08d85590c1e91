#!/usr/bin/env python
"""Time the per-gene similarity thresholds on the GPU: the thresholds-and-join tail of ``segger segment`` with
``thresholds="kernel"`` (``postprocess.gene_thresholds``, csrc/thresholds.hip) against ``thresholds="torch"``
(``postprocess.per_gene_thresholds``: two stable sorts, float64 copies, a vectorised fixed-point loop) on the same
synthetic deduplicated columns, already on the device, in one process.

Per size (``--rows``, default 10^6 and 10^7): ``rows`` transcripts over 500 genes whose sizes fall off as 1 / rank (the
largest gene holds about 15 % of the rows), a tenth unassigned, bimodal similarities.  The two routes are run alternately
``--runs`` times after one warm-up each at that size and the medians are reported:

* seconds: HIP events on the current stream around the call (both routes end in a wait for the device);
* peak bytes: ``torch.cuda.max_memory_allocated`` over the call minus what was allocated when it began (the inputs);
* how far the two routes' thresholds are apart, and whether the kernel route gives the same bits twice.

One JSON line; ``--out`` also writes it to a file (profiles/thresholds_rows_per_s.json is the committed measurement)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_GENES = 500


def make_columns(n: int, device, seed: int):
    g = torch.Generator(device=device).manual_seed(seed)
    weights = 1.0 / torch.arange(1, N_GENES + 1, device=device, dtype=torch.float64)
    cdf = (weights / weights.sum()).cumsum(0)
    gene = torch.searchsorted(cdf, torch.rand(n, generator=g, device=device, dtype=torch.float64)).clamp_(max=N_GENES - 1)
    hi = torch.rand(n, generator=g, device=device) < 0.6
    sim = torch.where(hi, 0.7 + 0.1 * torch.randn(n, generator=g, device=device),
                      0.1 + 0.15 * torch.randn(n, generator=g, device=device)).clamp_(-1, 1)
    cell = torch.randint(0, max(n // 100, 1), (n,), generator=g, device=device)
    cell = torch.where(torch.rand(n, generator=g, device=device) < 0.1, torch.full_like(cell, -1), cell)
    return {"row_index": torch.arange(n, device=device), "cell_encoding": cell, "similarity": sim, "gene": gene}


def phase(fn):
    """-> (result, seconds by HIP events, peak bytes above what was allocated at the start)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return out, start.elapsed_time(stop) / 1e3, torch.cuda.max_memory_allocated() - base


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="1000000,10000000", help="row counts, comma separated")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_thresholds.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import _lib
    from segger_amd.postprocess import _thresholds_and_join

    dev = torch.device("cuda:0")
    sizes = []
    for n in [int(s) for s in args.rows.split(",") if s]:
        cols = make_columns(n, dev, args.seed)
        torch.cuda.empty_cache()
        entry = {"rows": n, "n_genes": N_GENES, "input_bytes": torch.cuda.memory_allocated(),
                 "largest_gene_rows": int(torch.bincount(cols["gene"][cols["cell_encoding"] >= 0]).max()),
                 "kernel_workspace_bytes": int(_lib.load().segger_thresholds_workspace_bytes(n, N_GENES))}
        runs = {"kernel": [], "torch": []}
        for r in range(args.runs + 1):                               # run 0 warms both routes up at this size
            got, t_a, p_a = phase(lambda: _thresholds_and_join(dict(cols), 250, "kernel"))
            ref, t_b, p_b = phase(lambda: _thresholds_and_join(dict(cols), 250, "torch"))
            if r == 0:
                a, b = got["similarity_threshold"], ref["similarity_threshold"]
                entry["threshold_max_abs_diff"] = float((a - b)[~a.isnan()].abs().max())
                entry["nan_pattern_equal"] = bool(torch.equal(a.isnan(), b.isnan()))
                entry["failed_genes"] = [int(got["failed_genes"].numel()), int(ref["failed_genes"].numel())]
                first = a.clone()
            else:
                runs["kernel"].append((t_a, p_a))
                runs["torch"].append((t_b, p_b))
                entry["kernel_same_bits_every_run"] = bool(entry.get("kernel_same_bits_every_run", True) and torch.equal(
                    got["similarity_threshold"].view(torch.int64), first.view(torch.int64)))
            del got, ref
        for name, rs in runs.items():
            sec = statistics.median(t for t, _ in rs)
            entry[name] = {"seconds_median": sec, "seconds": [t for t, _ in rs], "rows_per_s": n / sec,
                           "peak_bytes_above_inputs": max(p for _, p in rs),
                           "peak_bytes_per_row": max(p for _, p in rs) / n}
        entry["seconds_ratio_torch_over_kernel"] = entry["torch"]["seconds_median"] / entry["kernel"]["seconds_median"]
        entry["peak_ratio_torch_over_kernel"] = (entry["torch"]["peak_bytes_above_inputs"]
                                                 / max(entry["kernel"]["peak_bytes_above_inputs"], 1))
        sizes.append(entry)
        print(f"[thresholds] {entry}", file=sys.stderr, flush=True)
        del cols, first
        torch.cuda.empty_cache()
    res = {"what": "thresholds-and-join tail: thresholds='kernel' (HIP, one keys-only sort) vs thresholds='torch' on synthetic rows",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "HIP events around the call; median of the runs after one warm-up; the two routes alternate; peak bytes "
                     "include the joined [rows] float64 threshold column both routes return (8 B per row)", "sizes": sizes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
