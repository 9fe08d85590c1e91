#!/usr/bin/env python
"""Time the cell boundary polygons on the GPU: ``boundaries.cell_boundaries`` (csrc/boundaries.hip: one keys-only sort,
one wave per cell; registers up to 64 transcripts, LDS up to 4096, the chunked route above) on synthetic segmentations
already on the device.

Workloads: ``--transcripts`` rows (default 10^6 and 10^7) at about 150 transcripts per cell, 1 % of the cells with 4100 ..
6000 (the chunked route), real slide coordinates, rows in random order; ``smoothing`` 0 and 2.  Per workload, after one
warm-up, ``--runs`` calls are timed and the median reported: the whole Python call by the host clock around a
synchronise (allocation, the call, the one wait for the counters), the C entry point alone by device events, and the
split of the device time over the stages (keys, sort and compaction, binning, the three hull kernels, scan, emit) from
the kernel records of ``torch.profiler`` over three further calls ("unavailable" if the profiler gives none).

The comparison figure is what a user has today: ``scipy.spatial.ConvexHull`` per cell on ``--cpu-procs`` processes
(default 16), timed on a SUBSAMPLE of ``--cpu-cells`` cells of the 10^6 workload, rows already grouped by cell, and scaled
to all its cells -- labelled as such.  The reference's loop is this plus a shapely call per cell; it was not run.

One JSON line; ``--out`` also writes it to a file (profiles/boundaries_cells_per_s.json is the committed measurement).
There is no pass / fail bar on speed."""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = (("keys", ("bnd_keys_kernel",)), ("sort_and_compaction", ("rocprim",)), ("bin", ("bnd_bin_kernel",)),
          ("hull_registers", ("bnd_short_kernel",)), ("hull_lds", ("bnd_long_kernel",)), ("hull_chunked", ("bnd_chunk_kernel",)),
          ("scan", ("bnd_scan_kernel",)), ("emit", ("bnd_emit_kernel",)))


def segmentation(n_rows: int, seed: int):
    """(xy [N, 2] float64, cell [N] int32, n_cells): ~150 transcripts per cell, 1 % of the cells 4100 .. 6000, shuffled"""
    rng = np.random.default_rng(seed)
    mean_all = 0.99 * 150 + 0.01 * 5050
    n_cells = max(int(n_rows / mean_all), 1)
    counts = np.maximum(rng.poisson(150, n_cells), 1)
    big = rng.choice(n_cells, max(n_cells // 100, 1), replace=False)
    counts[big] = rng.integers(4100, 6001, big.size)
    owner = np.repeat(np.arange(n_cells, dtype=np.int32), counts)
    sigma = np.where(counts > 4096, 20.0, 4.0)
    centre = rng.uniform(1e4, 9e4, (n_cells, 2))
    xy = centre[owner] + rng.normal(0.0, 1.0, (owner.size, 2)) * sigma[owner, None]
    perm = rng.permutation(owner.size)
    return np.ascontiguousarray(xy[perm]), owner[perm], n_cells


def _scipy_chunk(groups) -> int:
    from scipy.spatial import ConvexHull
    return sum(len(ConvexHull(p).vertices) for p in groups)


def cpu_scipy_rate(xy, cell, n_cells: int, n_sample: int, procs: int) -> dict:
    order = np.argsort(cell, kind="stable")
    bounds = np.searchsorted(cell[order], np.arange(n_cells + 1))
    pick = np.random.default_rng(1).choice(n_cells, min(n_sample, n_cells), replace=False)
    groups = [xy[order[bounds[c]:bounds[c + 1]]] for c in pick]
    chunks = [groups[i::procs * 4] for i in range(procs * 4)]
    with multiprocessing.get_context("fork").Pool(procs) as pool:
        pool.map(_scipy_chunk, chunks[:procs])                        # start the workers, import scipy
        t = time.perf_counter()
        pool.map(_scipy_chunk, chunks)
        dt = time.perf_counter() - t
    return {"what": "CPU figure: scipy.spatial.ConvexHull per cell, rows already grouped by cell; a SUBSAMPLE of the cells, "
                    "scaled to all of them",
            "processes": procs, "cells_timed": len(groups), "seconds": dt, "cells_per_s": len(groups) / dt,
            "scaled_seconds_for_all_cells": dt * n_cells / len(groups), "cells": n_cells, "transcripts": int(len(cell))}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--transcripts", default="1000000,10000000", help="row counts, comma separated")
    ap.add_argument("--smoothing", default="0,2")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--cpu-cells", type=int, default=4000, help="0 skips the CPU figure")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sizes = [int(s) for s in args.transcripts.split(",") if s]
    data = {n: segmentation(n, args.seed) for n in sizes}
    cpu = cpu_scipy_rate(*data[sizes[0]], args.cpu_cells, args.cpu_procs) if args.cpu_cells > 0 else None
    print(f"[boundaries] {cpu}", file=sys.stderr, flush=True)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_boundaries.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import _lib as L
    from segger_amd import boundaries as bd
    dev = torch.device("cuda:0")

    def stage_split(call) -> dict:
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
            us = {name: 0.0 for name, _ in STAGES}
            for ev in prof.events():
                dur = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
                for name, keys in STAGES:
                    if any(k in ev.name for k in keys):
                        us[name] += float(dur) / 3.0
                        break
            return {"ms_per_call": {k: v * 1e-3 for k, v in us.items()}} if sum(us.values()) > 0 else {"unavailable": "no kernel records"}
        except Exception as e:                                       # the split is an extra: the timings above stand without it
            return {"unavailable": repr(e)[:200]}

    workloads = []
    for n in sizes:
        xy_h, cell_h, n_cells = data[n]
        xy, cell = torch.from_numpy(xy_h).to(dev), torch.from_numpy(cell_h).to(dev)
        for s in [int(v) for v in args.smoothing.split(",") if v]:
            cap = min(n, n_cells)
            ring_offsets = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
            out = torch.empty(n << s, 2, dtype=torch.float64, device=dev)
            cell_ids, n_tx = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
            counters = torch.zeros(L.BOUNDARY_COUNTERS, dtype=torch.int64, device=dev)
            ws, ws_bytes = L.workspace("segger_cell_boundaries_workspace_bytes", dev, n, n_cells)

            def entry_point():
                L.call("segger_cell_boundaries", dev, xy.data_ptr(), cell.data_ptr(), None, n, n_cells, s, ring_offsets.data_ptr(),
                       out.data_ptr(), n << s, cell_ids.data_ptr(), n_tx.data_ptr(), counters.data_ptr(), ws.data_ptr(), ws_bytes)

            dev_ms, host_ms = [], []
            for r in range(args.runs + 1):                            # run 0 warms up
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                entry_point()
                stop.record()
                stop.synchronize()
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = bd.cell_boundaries(xy, cell, n_cells, smoothing=s)
                torch.cuda.synchronize()
                if r:
                    dev_ms.append(start.elapsed_time(stop))
                    host_ms.append((time.perf_counter() - t) * 1e3)
            c = dict(zip(bd.COUNTERS, counters.tolist()))
            words = ws[:16].view(torch.int32).tolist()
            assert c["n_counted"] == n and c["n_present"] == n_cells and c["n_refused"] == 0 and c["n_kept"] == int(res["cell_ids"].numel())
            med = statistics.median(dev_ms)
            entry = {"transcripts": n, "cells": n_cells, "smoothing": s, "polygons": c["n_kept"], "vertices": c["n_vertices"],
                     "register_route": words[1], "lds_route": words[2], "chunked_route": words[3],
                     "entry_point_ms_median_device_events": med, "entry_point_ms": dev_ms,
                     "python_call_ms_median_host_clock": statistics.median(host_ms), "python_call_ms": host_ms,
                     "cells_per_s": n_cells / (med * 1e-3), "transcripts_per_s": n / (med * 1e-3), "stages": stage_split(entry_point)}
            workloads.append(entry)
            print(f"[boundaries] {entry}", file=sys.stderr, flush=True)
            del out, ws, res
    res = {"what": "segger_cell_boundaries on synthetic segmentations: ~150 transcripts per cell, 1 % of the cells 4100 .. 6000",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "median of the runs after one warm-up; entry point: device events around the call; python call: host clock "
                     "around a synchronise; stages: torch.profiler kernel records, mean of three further calls",
           "not_measured": "the reference's generate_boundaries (geopandas, shapely and polars are not installed); the CPU figure "
                           "is scipy's hull alone, without the reference's per-cell shapely overhead and without the grouping",
           "cpu_comparison": cpu, "workloads": workloads}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
