#!/usr/bin/env python
"""Time the nearest boundaries on the GPU: ``nearest.nearest_boundaries`` (csrc/nearest_boundaries.hip: the join's walk
twice, a count and a fill of (key, polygon) per pair, and a selection of the k best per point) against two baselines run
in the same process on the same scenes:

* ``floor``: ``geometry.points_in_polygons(buffer=max_dist, "intersects")`` alone -- the same walk without distances or
  selection (it sorts its pair list by point, which the new unit does not);
* ``composition``: that join followed by what a user would write today in plain torch -- the distances and parities of
  its pairs from a padded vertex table, in chunks of ``--chunk`` pairs, the key s, and a sort-based top-k (a sort by s,
  a stable sort by point, the rank inside the point's run).

Scenes: those of tools/bench_polygon_join.py (13-vertex star rings about 10 um across on a jittered lattice, about 200
uniformly placed points per polygon) -- 10^6 points x 5 x 10^3 rings and 10^7 x 5 x 10^4 (``--points``) -- with ``--k`` 3
and ``max_dist`` 1 um and 6 um (``--dists``).  Per scene, after one warm-up, ``--runs`` calls of each route are timed with
device events around the whole Python call (its host synchronisations are inside) and the medians are reported, with the
peak device memory above the inputs (torch's allocator peak during one call) and the mean and maximum ``count``.  The
composition must keep the same polygons: checked once per scene and reported.

One JSON line; ``--out`` also writes it to a file (profiles/nearest_points_per_s.json is the committed measurement).
There is no pass / fail bar on speed, and nothing here says what bounds the kernels: that takes a counter run."""
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
    ap.add_argument("--dists", default="1.0,6.0", help="max_dist values, comma separated")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="pairs per chunk of the torch composition")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_nearest.py needs an MI355X: a CPU timing says nothing about it")
    from bench_polygon_join import slide
    from segger_amd import geometry as ge, nearest
    dev = torch.device("cuda:0")

    def vertex_table(o, v):
        """[P, nmax + 1, 2] open rings translated to their first vertex and closed by it, and their lengths"""
        n = o[1:] - o[:-1]
        last = v[(o[1:] - 1).clamp(min=0)]
        n = n - ((n > 1) & (last == v[o[:-1].clamp(max=v.shape[0] - 1)]).all(1)).long()      # a closing duplicate is dropped
        nmax = int(n.max())
        j = torch.arange(nmax + 1, device=dev)[None, :]
        idx = o[:-1, None] + torch.where(j < n[:, None], j, torch.zeros_like(j))             # beyond the ring: its first vertex
        return v[idx] - v[o[:-1], None, :], n, v[o[:-1]]

    def composition(pts, o, v, max_dist, k):
        ei = ge.points_in_polygons(pts, o, v, buffer=max_dist, predicate="intersects")
        table, n, first = vertex_table(o, v)
        E, P, N = ei.shape[1], o.numel() - 1, pts.shape[0]
        s = torch.empty(E, dtype=torch.float64, device=dev)
        inside = torch.empty(E, dtype=torch.bool, device=dev)
        edge = torch.arange(table.shape[1] - 1, device=dev)[None, :]
        for b in range(0, E, args.chunk):
            i, p = ei[0, b:b + args.chunk], ei[1, b:b + args.chunk]
            ring = table[p]
            a, c = ring[:, :-1], ring[:, 1:]
            t = (pts[i] - first[p])[:, None, :]
            ex, ey, wx, wy = c[..., 0] - a[..., 0], c[..., 1] - a[..., 1], t[..., 0] - a[..., 0], t[..., 1] - a[..., 1]
            cr, dot, len2 = ex * wy - ey * wx, wx * ex + wy * ey, ex * ex + ey * ey
            ux, uy = t[..., 0] - c[..., 0], t[..., 1] - c[..., 1]
            d2 = torch.where((dot <= 0) | (len2 == 0), wx * wx + wy * wy, torch.where(dot >= len2, ux * ux + uy * uy, cr * cr / len2))
            valid = edge < n[p][:, None]
            d2 = torch.where(valid, d2, torch.full_like(d2, float("inf"))).min(1).values
            a_below, b_below = a[..., 1] <= t[..., 1], c[..., 1] <= t[..., 1]
            cross = valid & ((a_below & ~b_below & (cr > 0)) | (~a_below & b_below & (cr < 0)))
            par = (cross.sum(1) & 1).bool()
            s[b:b + args.chunk] = torch.where(d2 == 0, torch.zeros_like(d2), torch.where(par, -d2, d2))
            inside[b:b + args.chunk] = par
        order = torch.sort(s, stable=True).indices                   # ei is sorted by (point, polygon): ties keep the lower id
        order = order[torch.sort(ei[0][order], stable=True).indices]
        point = ei[0][order]
        count = torch.bincount(point, minlength=N)
        start = torch.cumsum(count, 0) - count
        rank = torch.arange(E, device=dev) - start[point]
        keep = rank < k
        polygon = torch.full((N, k), P, dtype=torch.int32, device=dev)
        dist2 = torch.full((N, k), float("inf"), dtype=torch.float64, device=dev)
        ins = torch.zeros((N, k), dtype=torch.bool, device=dev)
        polygon[point[keep], rank[keep]] = ei[1][order][keep].int()
        dist2[point[keep], rank[keep]] = s[order][keep].abs()
        ins[point[keep], rank[keep]] = inside[order][keep]
        return {"polygon": polygon, "dist2": dist2, "inside": ins, "count": count.int()}

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

    def route(ms, all_ms, peak, N):
        return {"ms_median": ms, "ms": all_ms, "points_per_s": N / (ms * 1e-3), "peak_bytes_above_inputs": peak}

    scenes = []
    for N in [int(x) for x in args.points.split(",") if x]:
        points, offsets, xy = slide(N, 0.0, args.seed)
        pts, o, v = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (points, offsets, xy))
        for max_dist in [float(x) for x in args.dists.split(",") if x]:
            n_ms, n_all, n_peak, near = timed(lambda: nearest.nearest_boundaries(pts, o, v, args.k, buffer=max_dist))
            f_ms, f_all, f_peak, ei = timed(lambda: ge.points_in_polygons(pts, o, v, buffer=max_dist, predicate="intersects"))
            del ei
            c_ms, c_all, c_peak, comp = timed(lambda: composition(pts, o, v, max_dist, args.k))
            c = dict(zip(nearest.COUNTER_NAMES, near["counters"].tolist()))
            entry = {"points": N, "polygons": int(o.numel()) - 1, "k": args.k, "max_dist": max_dist, "pairs": c["n_pairs"],
                     "mean_count": c["n_pairs"] / N, "max_count": c["max_count"], "truncated_point_share": c["n_truncated_points"] / N,
                     "same_polygons_as_the_composition": bool(torch.equal(near["polygon"], comp["polygon"])),
                     "same_count_as_the_composition": bool(torch.equal(near["count"], comp["count"])),
                     "dist2_bit_equal_to_the_composition": bool(torch.equal(near["dist2"], comp["dist2"])),
                     "nearest": route(n_ms, n_all, n_peak, N), "floor_join": route(f_ms, f_all, f_peak, N),
                     "composition": route(c_ms, c_all, c_peak, N), "nearest_over_floor_time": n_ms / f_ms,
                     "nearest_over_composition_time": n_ms / c_ms, "composition_over_nearest_peak": c_peak / max(n_peak, 1),
                     "nearest_over_floor_peak": n_peak / max(f_peak, 1)}
            scenes.append(entry)
            print(f"[nearest] { {k: v for k, v in entry.items() if k not in ('nearest', 'floor_join', 'composition')} } "
                  f"nearest {n_ms:.3f} ms {n_peak} B  floor {f_ms:.3f} ms {f_peak} B  composition {c_ms:.3f} ms {c_peak} B",
                  file=sys.stderr, flush=True)
            del near, comp
    res = {"what": "nearest.nearest_boundaries (k best boundaries per point, predicate intersects, a uniform buffer max_dist) "
                   "against points_in_polygons alone (the floor) and against that join + a chunked plain-torch computation of its "
                   "pairs' distances + a sort-based top-k, on the synthetic slides of tools/bench_polygon_join.py: ~10 um 13-vertex "
                   "star rings, ~200 points per polygon",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed, "chunk": args.chunk,
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
