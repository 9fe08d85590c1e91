#!/usr/bin/env python
"""Time the route through global memory of the concave cell outlines (``segger_cell_outlines_large``,
csrc/outlines_large.hip) on the GPU, with the entry point, device events and the median of ``--runs`` calls after one
warm-up, as tools/bench_outlines.py does:

* one cell of 2049, 4096, 16 384 and 65 537 distinct points (uniform on the 1/16 grid, 2001 x 2001 steps) on the new route;
* one cell of 2048 points on the LDS route and, with ``lds_max_points = 0``, on the new one: the price of global memory;
* the 10^6-transcript / 5 10^3-cell scene of tools/bench_outlines.py through ``segger_cell_outlines`` (the default path),
  through the new entry point with nothing to route, and with one more cell of 10^4 points: what the one cell adds.

One JSON line; ``--out`` also writes it (profiles/outlines_large_cells.json is the committed measurement).  No bar is set."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--sizes", default="2049,4096,16384,65537")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_outlines_large.py needs an MI355X: a CPU timing says nothing about it")
    import outline_cases as oc
    from bench_outlines import segmentation
    from segger_amd import _lib as L
    from segger_amd import boundaries as bd
    dev = torch.device("cuda:0")

    def timed(xy_h, cell_h, n_cells, lds_max=None, large_rows=0):
        """median ms of the entry point (lds_max None: segger_cell_outlines) and its counters"""
        n = len(cell_h)
        xy, cell = torch.from_numpy(np.ascontiguousarray(xy_h)).to(dev), torch.from_numpy(cell_h.astype(np.int32)).to(dev)
        large = lds_max is not None
        names = bd.LARGE_OUTLINE_COUNTER_NAMES if large else bd.OUTLINE_COUNTER_NAMES
        _, offs, out, cell_ids, n_tx, counters = bd._outputs(dev, n, n_cells, 0, len(names))
        if large:
            ws, ws_bytes = L.workspace("segger_cell_outlines_large_workspace_bytes", dev, n, n_cells, large_rows)
            tail = (lds_max, large_rows)
        else:
            ws, ws_bytes = L.workspace("segger_cell_outlines_workspace_bytes", dev, n, n_cells)
            tail = ()
        ms = []
        for r in range(args.runs + 1):                                # run 0 warms up
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            L.call("segger_cell_outlines_large" if large else "segger_cell_outlines", dev, xy.data_ptr(), cell.data_ptr(), None, n,
                   n_cells, 2.0, 0, offs.data_ptr(), out.data_ptr(), n, cell_ids.data_ptr(), n_tx.data_ptr(), counters.data_ptr(),
                   ws.data_ptr(), ws_bytes, *tail)
            stop.record()
            stop.synchronize()
            if r:
                ms.append(start.elapsed_time(stop))
        c = dict(zip(names, counters.tolist()))
        assert c["n_refused"] == 0 and c["n_failed"] == 0, c
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "polygons": c["n_kept"],
                "vertices": c["n_vertices"], "large_cells": c.get("n_large_cells", 0), "large_points": c.get("n_large_points", 0)}

    res = {"what": "segger_cell_outlines_large: the route through global memory for cells above the LDS budget",
           "device": torch.cuda.get_device_name(0), "runs": args.runs,
           "timing": "device events around the entry point, median (and min, max) of the runs after one warm-up"}
    cells = []
    for d in (int(s) for s in args.sizes.split(",") if s):
        pts = oc.cloud(d, d, 1000)
        cells.append({"distinct_points": d, **timed(pts, np.zeros(d), 1, L.OUTLINE_MAX_POINTS, d)})
        print(f"[outlines_large] {cells[-1]}", file=sys.stderr, flush=True)
    res["one_cell_on_the_new_route"] = cells
    pts = oc.big_cells()[1]
    lds, glob = timed(pts, np.zeros(len(pts)), 1, L.OUTLINE_MAX_POINTS, 0), timed(pts, np.zeros(len(pts)), 1, 0, len(pts))
    res["cell_of_2048_points"] = {"lds_route": lds, "global_route": glob, "ratio": glob["ms_median"] / lds["ms_median"]}
    xy, cell, n_cells = segmentation(1000000, 0)
    per_cell = np.bincount(cell, minlength=n_cells)
    rows_above = int(per_cell[per_cell > L.OUTLINE_MAX_POINTS].sum())
    scene = {"transcripts": len(cell), "cells": n_cells, "default_entry_point": timed(xy, cell, n_cells),
             "large_entry_point_nothing_to_route": timed(xy, cell, n_cells, L.OUTLINE_MAX_POINTS, rows_above)}
    big = oc.cloud(10000, 10000, 1000) + [5e4, 5e4]
    xy2, cell2 = np.concatenate([xy, big]), np.concatenate([cell, np.full(len(big), n_cells, dtype=cell.dtype)])
    scene["large_entry_point_plus_one_cell_of_10000_points"] = timed(xy2, cell2, n_cells + 1, L.OUTLINE_MAX_POINTS,
                                                                     rows_above + len(big))
    scene["the_one_cell_alone"] = timed(big, np.zeros(len(big)), 1, L.OUTLINE_MAX_POINTS, len(big))
    scene["note"] = ("the large kernel starts when the LDS kernels are done: the call with the one cell costs about the scene plus the "
                     "cell alone")
    res["scene_1e6"] = scene
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
