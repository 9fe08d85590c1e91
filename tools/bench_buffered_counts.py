#!/usr/bin/env python
"""Time the buffered-boundary count matrix on the GPU: ``buffered_counts.buffered_counts`` (csrc/buffered_counts.hip: the
polygon join and the gene histogram fused, one wave per polygon, a count and a fill pass) against the composition it
replaces, run in the same process on the same scenes: ``geometry.points_in_polygons`` (the pair list and its sort by
point) followed by a torch sort and ``unique_consecutive`` of the ``polygon * n_genes + gene`` keys.

Scenes: those of tools/bench_polygon_join.py (13-vertex star rings about 10 um across on a jittered lattice, about 200
uniformly placed points per polygon) -- 10^6 points x 5 x 10^3 rings and 10^7 x 5 x 10^4 (``--points``) -- at buffer 0 and
at ``--buffer`` (default 6 um: the mean point then lies in about three grown polygons; the measured mean is reported), at
``--genes`` 500 and 5000, uniformly drawn.  Per scene, after one warm-up, ``--runs`` calls of each route are timed with
device events around the whole Python call (its host synchronisations are inside) and the medians are reported, with the
peak device memory above the inputs (torch's allocator peak during one call) and the share of rows on the overflow path.
Both routes must give the same matrix: checked once per scene.

One JSON line; ``--out`` also writes it to a file (profiles/buffered_counts_points_per_s.json is the committed
measurement).  There is no pass / fail bar on speed, and nothing here says what bounds the kernels: that takes a counter
run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default="1000000,10000000", help="point counts, comma separated")
    ap.add_argument("--genes", default="500,5000", help="panel sizes, comma separated")
    ap.add_argument("--buffer", type=float, default=6.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_buffered_counts.py needs an MI355X: a CPU timing says nothing about it")
    from bench_polygon_join import slide
    from segger_amd import buffered_counts as bcm, geometry as ge
    dev = torch.device("cuda:0")

    def composition(pts, gene, o, v, n_genes, buffer):
        ei = ge.points_in_polygons(pts, o, v, buffer=buffer)
        key = torch.sort(ei[1] * n_genes + gene[ei[0]]).values
        uniq, counts = torch.unique_consecutive(key, return_counts=True)
        row = torch.div(uniq, n_genes, rounding_mode="floor")
        indptr = torch.zeros(o.numel(), dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(row, minlength=o.numel() - 1), 0, out=indptr[1:])
        return {"indptr": indptr, "indices": (uniq - row * n_genes).to(torch.int32), "counts": counts.to(torch.int32)}

    def timed(fn) -> tuple:
        ms, peak, out = [], 0, None
        for r in range(args.runs + 1):                                # run 0 warms up
            out = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = fn()
            stop.record()
            stop.synchronize()
            peak = max(peak, torch.cuda.max_memory_allocated(dev) - base)
            if r:
                ms.append(start.elapsed_time(stop))
        return statistics.median(ms), ms, int(peak), out

    scenes = []
    for N in [int(s) for s in args.points.split(",") if s]:
        points, offsets, xy = slide(N, 0.0, args.seed)
        pts, o, v = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (points, offsets, xy))
        for n_genes in [int(s) for s in args.genes.split(",") if s]:
            gene = torch.from_numpy(np.random.default_rng(args.seed + 1).integers(0, n_genes, N)).to(dev)
            for buffer in (0.0, args.buffer):
                f_ms, f_all, f_peak, fused = timed(lambda: bcm.buffered_counts(pts, gene, o, v, n_genes, buffer=buffer))
                c_ms, c_all, c_peak, comp = timed(lambda: composition(pts, gene, o, v, n_genes, buffer))
                same = all(torch.equal(fused[k], comp[k]) for k in ("indptr", "indices", "counts"))
                c = dict(zip(bcm.COUNTER_NAMES, fused["counters"].tolist()))
                P = int(o.numel()) - 1
                entry = {"points": N, "polygons": P, "n_genes": n_genes, "buffer": buffer, "pairs": c["n_pairs"], "nnz": c["nnz"],
                         "mean_polygons_per_point": c["n_pairs"] / N, "same_matrix_as_the_composition": same,
                         "fused": {"ms_median": f_ms, "ms": f_all, "points_per_s": N / (f_ms * 1e-3), "peak_bytes_above_inputs": f_peak},
                         "composition": {"ms_median": c_ms, "ms": c_all, "points_per_s": N / (c_ms * 1e-3),
                                         "peak_bytes_above_inputs": c_peak},
                         "fused_over_composition_time": f_ms / c_ms, "composition_over_fused_peak": c_peak / max(f_peak, 1),
                         "overflow_row_share": c["n_overflow_rows"] / P, "large_tier_rows": c["n_large_tier"]}
                scenes.append(entry)
                print(f"[buffered_counts] { {k: v for k, v in entry.items() if k not in ('fused', 'composition')} } "
                      f"fused {f_ms:.3f} ms {f_peak} B  composition {c_ms:.3f} ms {c_peak} B", file=sys.stderr, flush=True)
                del fused, comp
    res = {"what": "buffered_counts.buffered_counts (predicate contains) against points_in_polygons + torch sort / "
                   "unique_consecutive of polygon * n_genes + gene, on the synthetic slides of tools/bench_polygon_join.py: ~10 um "
                   "13-vertex star rings, ~200 points per polygon, genes drawn uniformly",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "device events around the whole Python call (host synchronisations included); median of the runs after one "
                     "warm-up; peak = torch's allocator peak above the inputs during one call",
           "what_bounds_the_kernels": "not measured (no counter run was made)", "scenes": scenes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
