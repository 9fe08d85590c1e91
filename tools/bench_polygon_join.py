#!/usr/bin/env python
"""Time the shape-based prediction graph on the GPU: ``neighbors.prediction_graph_shape`` -> ``geometry.points_in_polygons``
(csrc/polygon_join.hip: points binned into a uniform grid, one wave per polygon, a count and a fill pass) on a synthetic
slide, already on the device.

Workloads: 13-vertex star rings about 10 um across on a jittered lattice with about 200 uniformly placed points per
polygon, at the default buffer ratio 0.05 -- 10^6 points with 5 x 10^3 polygons and 10^7 points with 5 x 10^4 polygons
(``--points``) -- and at each size a mix with 1 % rings of 200 .. 2000 vertices.  Per workload, after one warm-up,
``--runs`` calls are timed with device events and the medians are reported: around the whole Python call (validation,
the polygon areas, the grid, both C calls, the final sort by point: its host synchronisations are inside), and around the
two C entry points alone (segger_polygon_join_count: keys, sort, cells, binning, count pass, scan;
segger_polygon_join_fill: the fill pass).  Peak device memory above the inputs is torch's allocator peak during one call.

For scale, a chunked plain-torch formulation of the same predicate on the smaller 13-vertex workload
(``--torch-points``): for each chunk of polygons the candidates are the points inside the chunk's bounding boxes grown by
d (a dense comparison against every point, written below), then parity and dist2 as dense [candidates, 13] tensors.

One JSON line; ``--out`` also writes it to a file (profiles/polygon_join_points_per_s.json is the committed measurement).
There is no pass / fail bar on speed, and nothing here says what bounds the kernels: that takes a counter run."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLIDE = (30000.25, 90000.5)
POINTS_PER_POLYGON = 200


def slide(n_points: int, long_fraction: float, seed: int):
    """(points [N, 2], ring_offsets [P + 1], xy [V, 2]) float64 numpy: P = N / 200 rings on a jittered 10 um lattice"""
    rng = np.random.default_rng(seed)
    P = max(n_points // POINTS_PER_POLYGON, 1)
    per_row = int(math.ceil(math.sqrt(P)))
    side = 10.0 * per_row
    counts = np.full(P, 13, dtype=np.int64)
    if long_fraction > 0:
        long_ids = rng.choice(P, max(int(P * long_fraction), 1), replace=False)
        counts[long_ids] = rng.integers(200, 2001, long_ids.size)
    offsets = np.zeros(P + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    owner = np.repeat(np.arange(P), counts)
    k = np.arange(offsets[-1]) - offsets[owner]
    ang = 2 * np.pi * (k + rng.uniform(0.0, 0.9, k.size)) / counts[owner]
    r = rng.uniform(4.0, 6.5, P)[owner] * rng.uniform(0.4, 1.0, k.size)
    ids = np.arange(P)
    centre = np.asarray(SLIDE) + (np.stack([ids % per_row, ids // per_row], 1) + 0.5) * 10.0 + rng.uniform(-2.0, 2.0, (P, 2))
    xy = centre[owner] + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    points = np.asarray(SLIDE) + rng.uniform(0.0, side, (n_points, 2))
    return points, offsets, xy


def torch_join(torch, points, rings, d, chunk: int = 64):
    """the same predicate in plain torch for rings of one length: rings [P, n, 2], d [P] -> number of pairs"""
    P, n, _ = rings.shape
    lo, hi = rings.min(1).values - d[:, None], rings.max(1).values + d[:, None]
    total = 0
    for s in range(0, P, chunk):
        e = min(s + chunk, P)
        inside = ((points[None, :, 0] >= lo[s:e, None, 0]) & (points[None, :, 0] <= hi[s:e, None, 0]) &
                  (points[None, :, 1] >= lo[s:e, None, 1]) & (points[None, :, 1] <= hi[s:e, None, 1]))
        poly, pt = inside.nonzero(as_tuple=True)
        poly = poly + s
        a = rings[poly] - rings[poly, :1]                             # [C, n, 2], translated to the first vertex
        b = torch.roll(a, -1, 1)
        t = (points[pt] - rings[poly, 0])[:, None, :]
        ex, ey, wx, wy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], t[..., 0] - a[..., 0], t[..., 1] - a[..., 1]
        cr, dot, len2 = ex * wy - ey * wx, wx * ex + wy * ey, ex * ex + ey * ey
        a_below, b_below = a[..., 1] <= t[..., 1], b[..., 1] <= t[..., 1]
        parity = (((a_below & ~b_below & (cr > 0)) | (~a_below & b_below & (cr < 0))).sum(1) & 1).bool()
        ux, uy = t[..., 0] - b[..., 0], t[..., 1] - b[..., 1]
        d2 = torch.where((dot <= 0) | (len2 == 0), wx * wx + wy * wy, torch.where(dot >= len2, ux * ux + uy * uy, cr * cr / len2))
        dist2 = d2.min(1).values
        total += int(((dist2 < d[poly] * d[poly]) | (parity & (dist2 > 0))).sum())
    return total


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", default="1000000,10000000", help="point counts, comma separated")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--torch-points", type=int, default=1000000, help="0 skips the plain-torch figure")
    ap.add_argument("--torch-runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_polygon_join.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import _lib as L, morphology as mo, neighbors as nb
    dev = torch.device("cuda:0")

    inner = {}
    plain_call = L.call

    def timed_call(fn_name, device, *a):                              # device events around the two C entry points
        if not fn_name.startswith("segger_polygon_join_"):
            return plain_call(fn_name, device, *a)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        plain_call(fn_name, device, *a)
        stop.record()
        inner.setdefault(fn_name, []).append((start, stop))

    def timed(points, offsets, xy) -> dict:
        pts, o, v = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (points, offsets, xy))
        N, P, V = int(pts.shape[0]), int(o.numel()) - 1, int(v.shape[0])
        whole, count_ms, fill_ms, peak, pairs = [], [], [], 0, 0
        L.call = timed_call
        try:
            for r in range(args.runs + 1):                            # run 0 warms up
                inner.clear()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                ei = nb.prediction_graph_shape(pts, o, v)
                stop.record()
                stop.synchronize()
                peak = max(peak, torch.cuda.max_memory_allocated(dev) - base)
                pairs = int(ei.shape[1])
                del ei
                if r:
                    whole.append(start.elapsed_time(stop))
                    count_ms.append(sum(a.elapsed_time(b) for a, b in inner["segger_polygon_join_count"]))
                    fill_ms.append(sum(a.elapsed_time(b) for a, b in inner["segger_polygon_join_fill"]))
        finally:
            L.call = plain_call
        med = statistics.median(whole)
        kernels = statistics.median([c + f for c, f in zip(count_ms, fill_ms)])
        return {"points": N, "polygons": P, "vertices": V, "pairs": pairs, "ms_whole_call_median": med, "ms_whole_call": whole,
                "ms_count_plus_fill_median": kernels, "ms_count_median": statistics.median(count_ms),
                "ms_fill_median": statistics.median(fill_ms), "points_per_s_whole_call": N / (med * 1e-3),
                "points_per_s_count_plus_fill": N / (kernels * 1e-3), "peak_bytes_above_inputs": int(peak)}

    workloads = []
    for N in [int(s) for s in args.points.split(",") if s]:
        for name, frac in (("star13", 0.0), ("mix 99 % star13 + 1 % of 200 .. 2000 vertices", 0.01)):
            entry = {"workload": name, **timed(*slide(N, frac, args.seed))}
            workloads.append(entry)
            print(f"[polygon_join] {entry}", file=sys.stderr, flush=True)

    plain = None
    if args.torch_points > 0:
        points, offsets, xy = slide(args.torch_points, 0.0, args.seed)
        pts, o, v = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (points, offsets, xy))
        area = mo.polygon_props(o, v)["area"]
        d = torch.sqrt(area / math.pi) * 0.05
        rings = v.view(-1, 13, 2)
        ms, pairs = [], 0
        for r in range(args.torch_runs + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            pairs = torch_join(torch, pts, rings, d)
            stop.record()
            stop.synchronize()
            if r:
                ms.append(start.elapsed_time(stop))
        want = next(w["pairs"] for w in workloads if w["workload"] == "star13" and w["points"] == args.torch_points) \
            if any(w["workload"] == "star13" and w["points"] == args.torch_points for w in workloads) else None
        plain = {"what": "chunked plain torch (float64), 64 polygons per chunk, candidates from the grown bounding boxes against "
                         "every point; counts the pairs, does not order them", "points": args.torch_points,
                 "polygons": int(rings.shape[0]), "pairs": pairs, "pairs_of_the_kernels": want, "ms_median": statistics.median(ms),
                 "ms": ms, "points_per_s": args.torch_points / (statistics.median(ms) * 1e-3)}
        print(f"[polygon_join] {plain}", file=sys.stderr, flush=True)
    res = {"what": "neighbors.prediction_graph_shape (buffer ratio 0.05, predicate contains) on a synthetic slide: ~10 um star "
                   "rings, ~200 points per polygon",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "device events; median of the runs after one warm-up; whole call = the Python function with its host "
                     "synchronisations, count + fill = the two C entry points",
           "plain_torch": plain, "workloads": workloads}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
