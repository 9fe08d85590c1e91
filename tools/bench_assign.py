#!/usr/bin/env python
"""Time the streaming transcript -> cell assignment on the GPU: ``postprocess.SegmentationAccumulator``
(csrc/assign.hip) against ``postprocess.best_assignment`` on the same synthetic prediction rows, no model involved.

Per slide size (``--n-tx``, default 1M / 10M / 100M transcripts): ``--overlap`` x n_tx rows (every transcript once plus
random repeats, as overlapping prediction tiles produce them; similarities rounded to fp16 so that ties occur), shuffled
and cut into batches of ``--rows-per-batch``.  Both paths see the same batches in the same order, already on the device;
the two are run alternately ``--runs`` times after one warm-up each and the medians are reported:

* seconds: a host clock around work that ends in a device synchronise (accumulator: every ``update`` plus ``result()``;
  best_assignment: the call);
* peak bytes: ``torch.cuda.max_memory_allocated`` over the phase minus what was allocated when it began -- the input
  batches, reported as ``input_bytes``.  best_assignment needs all of them at once on top of its peak; the accumulator
  reads a batch once, so a caller that streams holds one batch at a time;
* whether the two results are equal.

One JSON line; ``--out`` also writes it to a file (profiles/assign_stream.json is the committed measurement)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_rows(n_tx: int, overlap: float, rows_per_batch: int, device, seed: int):
    """-> list of (tx_index i64, seg_idx i64, max_sim f32, gene_id i32) batches on ``device``."""
    g = torch.Generator(device=device).manual_seed(seed)
    extra = int(round((overlap - 1.0) * n_tx))
    tx = torch.cat([torch.arange(n_tx, device=device), torch.randint(0, n_tx, (extra,), generator=g, device=device)])
    tx = tx[torch.randperm(tx.numel(), generator=g, device=device)]
    n = int(tx.numel())
    sim = (torch.rand(n, generator=g, device=device) * 2 - 1).half().float()
    seg = torch.randint(0, 200_000, (n,), generator=g, device=device)
    seg = torch.where(torch.rand(n, generator=g, device=device) < 0.1, torch.full_like(seg, -1), seg)
    gene = torch.randint(0, 500, (n,), generator=g, device=device, dtype=torch.int32)
    cols = (tx, seg, sim, gene)
    return [tuple(c[o:o + rows_per_batch].clone() for c in cols) for o in range(0, n, rows_per_batch)]


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
    ap.add_argument("--n-tx", default="1000000,10000000,100000000", help="slide sizes, comma separated")
    ap.add_argument("--overlap", type=float, default=1.3, help="rows per transcript")
    ap.add_argument("--rows-per-batch", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_assign.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd.postprocess import SegmentationAccumulator, best_assignment

    dev = torch.device("cuda:0")

    def streamed(batches, n_tx):
        acc = SegmentationAccumulator(n_tx, dev)
        for b in batches:
            acc.update(*b)
        return acc.result()

    sizes = []
    for n_tx in [int(s) for s in args.n_tx.split(",") if s]:
        batches = make_rows(n_tx, args.overlap, args.rows_per_batch, dev, args.seed)
        rows = sum(int(b[0].numel()) for b in batches)
        torch.cuda.empty_cache()
        input_bytes = torch.cuda.memory_allocated()
        runs = {"accumulator": [], "best_assignment": []}
        equal = None
        for r in range(args.runs + 1):                               # run 0 warms both paths up at this size
            got, t_a, p_a = phase(lambda: streamed(batches, n_tx))
            ref, t_b, p_b = phase(lambda: best_assignment(batches, device=dev))
            if r == 0:
                equal = all(torch.equal(got[k], ref[k]) for k in ("row_index", "cell_encoding", "gene")) and bool(
                    ((got["similarity"] == ref["similarity"]) | (got["similarity"].isnan() & ref["similarity"].isnan())).all())
            else:
                runs["accumulator"].append((t_a, p_a))
                runs["best_assignment"].append((t_b, p_b))
            del got, ref
        entry = {"n_tx": n_tx, "rows": rows, "batches": len(batches), "input_bytes": input_bytes, "equal": bool(equal)}
        for name, rs in runs.items():
            sec = statistics.median(t for t, _ in rs)
            entry[name] = {"seconds_median": sec, "seconds": [t for t, _ in rs], "rows_per_s": rows / sec,
                           "peak_bytes_above_inputs": max(p for _, p in rs)}
        entry["accumulator"]["state_bytes"] = 16 * n_tx + 16
        entry["seconds_ratio_best_over_accumulator"] = entry["best_assignment"]["seconds_median"] / entry["accumulator"]["seconds_median"]
        entry["peak_ratio_best_over_accumulator"] = (entry["best_assignment"]["peak_bytes_above_inputs"]
                                                     / max(entry["accumulator"]["peak_bytes_above_inputs"], 1))
        sizes.append(entry)
        print(f"[assign] {entry}", file=sys.stderr, flush=True)
        del batches
        torch.cuda.empty_cache()
    res = {"what": "SegmentationAccumulator vs best_assignment on synthetic rows", "device": torch.cuda.get_device_name(0),
           "overlap": args.overlap, "rows_per_batch": args.rows_per_batch, "runs": args.runs, "seed": args.seed,
           "timing": "host clock around work ending in a device synchronise; median of the runs after one warm-up",
           "sizes": sizes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
