#!/usr/bin/env python
"""Time the concave cell outlines on the GPU: ``segger_cell_outlines`` (csrc/outlines.hip: one keys-only sort, then one
single-wave workgroup per cell: Delaunay, two peels, components, ring walk in LDS) on synthetic segmentations already on
the device.

Workloads: ``--transcripts`` rows (default 10^6 and 10^7) at about 200 transcripts per cell (10^6 / 5 10^3 and
10^7 / 5 10^4), Gaussian cells on slide scale snapped to a 1/16 grid (so that the CPU oracle of tests/outline_cases.py can
run on the same rows), rows in random order, connectivity 2.0, no smoothing.  Per workload, after one warm-up, ``--runs``
calls of the C entry point are timed with device events and the median reported, with the share of the sort and compaction
from the kernel records of ``torch.profiler`` over three further calls ("unavailable" if the profiler gives none).

The comparison figure is the CPU oracle -- ``scipy.spatial.Delaunay`` plus the reference's prune restated in Python and
the ring of the largest component -- per cell on ``--cpu-procs`` processes (default 16), timed on a SUBSAMPLE of
``--cpu-cells`` cells of the first workload, rows already grouped by cell, and scaled to all its cells -- labelled as
such.  The reference's own loop (shapely ``polygonize`` per cell) was NOT run: shapely is not installed.

One JSON line; ``--out`` also writes it to a file (profiles/outlines_cells_per_s.json is the committed measurement).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGES = (("keys", ("bnd_keys_kernel",)), ("sort_and_compaction", ("rocprim",)), ("bin", ("out_bin_kernel",)),
          ("cells_small_route", ("out_cell_kernelILi256", "out_cell_kernel<256")), ("cells_large_route", ("out_cell_kernel",)),
          ("scan", ("bnd_scan_kernel",)), ("emit", ("bnd_emit_kernel",)))


def segmentation(n_rows: int, seed: int):
    """(xy [N, 2] float64 on the 1/16 grid, cell [N] int32, n_cells): ~200 transcripts per cell, shuffled"""
    rng = np.random.default_rng(seed)
    n_cells = max(n_rows // 200, 1)
    counts = np.maximum(rng.poisson(200, n_cells), 3)
    owner = np.repeat(np.arange(n_cells, dtype=np.int32), counts)
    centre = rng.uniform(1e4, 9e4, (n_cells, 2))
    xy = np.round((centre[owner] + rng.normal(0.0, 4.0, (owner.size, 2))) * 16.0) / 16.0
    perm = rng.permutation(owner.size)
    return np.ascontiguousarray(xy[perm]), owner[perm], n_cells


def _oracle_chunk(groups) -> int:
    import outline_cases as oc
    return sum(0 if (r := oc.outline(p, 2.0)) is None else len(r) for p in groups)


def cpu_oracle_rate(xy, cell, n_cells: int, n_sample: int, procs: int) -> dict:
    order = np.argsort(cell, kind="stable")
    bounds = np.searchsorted(cell[order], np.arange(n_cells + 1))
    pick = np.random.default_rng(1).choice(n_cells, min(n_sample, n_cells), replace=False)
    groups = [xy[order[bounds[c]:bounds[c + 1]]] for c in pick]
    chunks = [groups[i::procs * 4] for i in range(procs * 4)]
    with multiprocessing.get_context("fork").Pool(procs) as pool:
        pool.map(_oracle_chunk, [g[:1] for g in chunks[:procs]])      # start the workers, import scipy
        t = time.perf_counter()
        pool.map(_oracle_chunk, chunks)
        dt = time.perf_counter() - t
    return {"what": "CPU figure: the oracle of tests/outline_cases.py (scipy Delaunay + the reference's prune restated in Python + "
                    "the ring) per cell, rows already grouped by cell; a SUBSAMPLE of the cells, scaled to all of them",
            "processes": procs, "cells_timed": len(groups), "seconds": dt, "cells_per_s": len(groups) / dt,
            "scaled_seconds_for_all_cells": dt * n_cells / len(groups), "cells": n_cells, "transcripts": int(len(cell))}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--transcripts", default="1000000,10000000", help="row counts, comma separated")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--cpu-cells", type=int, default=800, help="0 skips the CPU figure")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    sizes = [int(s) for s in args.transcripts.split(",") if s]
    data = {n: segmentation(n, args.seed) for n in sizes}
    cpu = cpu_oracle_rate(*data[sizes[0]], args.cpu_cells, args.cpu_procs) if args.cpu_cells > 0 else None
    print(f"[outlines] {cpu}", file=sys.stderr, flush=True)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_outlines.py needs an MI355X: a CPU timing says nothing about it")
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
        n = len(cell_h)
        xy, cell = torch.from_numpy(xy_h).to(dev), torch.from_numpy(cell_h).to(dev)
        cap = min(n, n_cells)
        ring_offsets = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        out = torch.empty(n, 2, dtype=torch.float64, device=dev)
        cell_ids, n_tx = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
        counters = torch.zeros(L.OUTLINE_COUNTERS, dtype=torch.int64, device=dev)
        ws, ws_bytes = L.workspace("segger_cell_outlines_workspace_bytes", dev, n, n_cells)

        def entry_point():
            L.call("segger_cell_outlines", dev, xy.data_ptr(), cell.data_ptr(), None, n, n_cells, 2.0, 0, ring_offsets.data_ptr(),
                   out.data_ptr(), n, cell_ids.data_ptr(), n_tx.data_ptr(), counters.data_ptr(), ws.data_ptr(), ws_bytes)

        dev_ms = []
        for r in range(args.runs + 1):                                # run 0 warms up
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            entry_point()
            stop.record()
            stop.synchronize()
            if r:
                dev_ms.append(start.elapsed_time(stop))
        c = dict(zip(bd.OUTLINE_COUNTER_NAMES, counters.tolist()))
        words = ws[:16].view(torch.int32).tolist()
        assert c["n_counted"] == n and c["n_present"] == n_cells and c["n_refused"] == 0 and c["n_failed"] == 0, c
        med = statistics.median(dev_ms)
        stages = stage_split(entry_point)
        sort_ms = stages.get("ms_per_call", {}).get("sort_and_compaction")
        entry = {"transcripts": n, "cells": n_cells, "connectivity": 2.0, "polygons": c["n_kept"], "vertices": c["n_vertices"],
                 "small_route": words[1], "large_route": words[2], "entry_point_ms_median_device_events": med, "entry_point_ms": dev_ms,
                 "cells_per_s": n_cells / (med * 1e-3), "transcripts_per_s": n / (med * 1e-3), "stages": stages,
                 "sort_share": None if sort_ms is None else sort_ms / med}
        workloads.append(entry)
        print(f"[outlines] {entry}", file=sys.stderr, flush=True)
        del out, ws
    res = {"what": "segger_cell_outlines on synthetic segmentations: ~200 transcripts per cell on a 1/16 grid, connectivity 2.0",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "median of the runs after one warm-up; entry point: device events around the call; stages: torch.profiler kernel "
                     "records, mean of three further calls",
           "not_measured": "the reference's generate_boundaries (geopandas, shapely and polars are not installed); the CPU figure is "
                           "scipy's Delaunay plus a Python restatement of the prune, without shapely's polygonize and the grouping",
           "cpu_comparison": cpu, "workloads": workloads}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
