#!/usr/bin/env python
"""Time ``rasterize.rasterize_rings`` (csrc/rasterize.hip: one wave per polygon, blocks of pixels filled or skipped whole)
on the GPU against the composition a user would write without it, in the same process on the same scenes:
``geometry.points_in_polygons`` over ALL H x W pixel centres, then the lowest polygon of every pixel scattered into an image.

Scenes:
  rings13_2048   5 x 10^3 13-vertex star rings (about 26 pixels across) on a jittered lattice, 2048 x 2048;
  rings13_8192   5 x 10^4 of them on 8192 x 8192;
  outlines_1m    the ``cell_outlines`` rings of tools/bench_outlines.py's 10^6-transcript segmentation (5 x 10^3 cells about 16 um
                 across on an 80 mm field) on 8192 x 8192 at 9.765625 um a pixel: polygons of a few pixels each;
  ring4096       one 4096-vertex star ring covering about 10^6 pixels of 2048 x 2048.
Per scene, after one warm-up, ``--runs`` calls are timed with device events around the whole Python call (its host
synchronisations are inside) and the medians reported: the block sides 4, 8 and 16, ``_block=1`` (the shortcut off), and the
composition (``--composition-runs``; its pair list is as large as the covered area, so the large scenes get fewer runs),
with the peak device memory above the inputs (torch's allocator peak during one call).  The images must be equal: checked
once per scene.  ring4096 is capped at 3 runs and 1 composition run (one wave walks the one ring: a call takes seconds);
every scene records the counts it used.  The CPU figure is the numpy oracle of tests/rasterize_cases.py (the per-polygon
masks) on ``--cpu-procs`` fresh processes over a SUBSAMPLE, scaled to the whole: ``--cpu-polygons`` of the polygons, or, for
the one-ring scene, ``--cpu-procs`` bands of 8 pixel rows out of the rows the ring spans.

One JSON line; ``--out`` also writes it to a file (profiles/rasterize_pixels_per_s.json is the committed measurement).  No
pass / fail bar on speed, and nothing here says what bounds the kernels: that takes a counter run."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCKS = (4, 8, 16)
RUN_CAPS = {"ring4096": (3, 1)}          # (runs, composition runs) at most: one wave walks the one ring, a call takes seconds


def star_rings(n_rings: int, size: int, seed: int):
    """13-vertex star rings on a jittered lattice that fills size x size pixels, their radius 0.45 of the lattice step"""
    rng = np.random.default_rng(seed)
    per_row = int(np.ceil(np.sqrt(n_rings)))
    step = size / per_row
    k = np.arange(n_rings)
    centre = (np.stack([k % per_row, k // per_row], 1) + 0.5) * step + rng.uniform(-0.1, 0.1, (n_rings, 2)) * step
    ang = np.sort(rng.uniform(0.0, 2 * np.pi, (n_rings, 13)), axis=1)
    r = 0.45 * step * rng.uniform(0.4, 1.0, (n_rings, 13))
    xy = centre[:, None, :] + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=2)
    return np.arange(n_rings + 1, dtype=np.int64) * 13, np.round(xy.reshape(-1, 2) * 1024) / 1024


def big_ring(size: int, seed: int):
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, 2 * np.pi, 4096))
    r = 0.3 * size * rng.uniform(0.85, 1.0, 4096)                    # about pi (0.28 size)^2 = 10^6 pixels at 2048
    xy = size / 2 + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    return np.array([0, 4096], np.int64), np.round(xy * 1024) / 1024


def _oracle_chunk(job) -> int:
    import rasterize_cases as rc
    rings, shape, scale, translation = job
    return sum(len(m["intersects"]) for m in rc.masks_f64(rings, shape, scale, translation))


def cpu_oracle(offsets, xy, shape, scale, translation, n_sample: int, procs: int) -> dict:
    P = len(offsets) - 1
    if P >= procs:
        pick = np.random.default_rng(1).choice(P, min(n_sample, P), replace=False)
        rings = [xy[offsets[p]:offsets[p + 1]] for p in pick]
        jobs = [(rings[i::procs], shape, scale, translation) for i in range(procs)]
        timed, whole, unit = len(rings), P, "polygons"
    else:                                                            # few huge rings: bands of 8 rows, spread over the rows they span
        rows = np.arange(shape[0]) * scale[1] + translation[1]
        span = np.flatnonzero((rows >= xy[:, 1].min()) & (rows <= xy[:, 1].max()))
        starts = span[0] + (np.arange(procs) * max((len(span) - 8) // procs, 1))
        rings = [xy[offsets[p]:offsets[p + 1]] for p in range(P)]
        jobs = [(rings, (8, shape[1]), scale, (translation[0], float(rows[r]))) for r in starts]
        timed, whole, unit = 8 * procs, len(span), "pixel_rows"
    with multiprocessing.get_context("spawn").Pool(procs) as pool:   # fresh processes: the parent may have the GPU open
        pool.map(_oracle_chunk, [(j[0][:1], (1, 1), scale, translation) for j in jobs])     # start the workers
        t = time.perf_counter()
        pool.map(_oracle_chunk, jobs)
        dt = time.perf_counter() - t
    return {"processes": procs, "unit": unit, "timed": timed, "whole": int(whole), "seconds": dt, "scaled_seconds_for_the_scene": dt * whole / timed}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="rings13_2048,rings13_8192,outlines_1m,ring4096")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--composition-runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--cpu-polygons", type=int, default=64, help="0 skips the CPU figure")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    names = [s for s in args.scenes.split(",") if s]

    host = {}
    for name in names:
        if name == "rings13_2048":
            host[name] = (*star_rings(5000, 2048, args.seed), (2048, 2048), (1.0, 1.0), (0.0, 0.0))
        elif name == "rings13_8192":
            host[name] = (*star_rings(50000, 8192, args.seed), (8192, 8192), (1.0, 1.0), (0.0, 0.0))
        elif name == "ring4096":
            host[name] = (*big_ring(2048, args.seed), (2048, 2048), (1.0, 1.0), (0.0, 0.0))
        elif name != "outlines_1m":
            raise SystemExit(f"unknown scene {name}")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rasterize.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import boundaries as bd, geometry as ge, rasterize as rm
    dev = torch.device("cuda:0")

    def composition(o, v, shape, scale, translation):
        H, W = shape
        cols = torch.arange(W, dtype=torch.float64, device=dev) * scale[0] + translation[0]
        rows = torch.arange(H, dtype=torch.float64, device=dev) * scale[1] + translation[1]
        pts = torch.stack([cols.repeat(H), rows.repeat_interleave(W)], dim=1)
        pairs = ge.points_in_polygons(pts, o, v, None, "intersects")  # sorted by (point, polygon)
        first = torch.ones(pairs.shape[1], dtype=torch.bool, device=dev)
        first[1:] = pairs[0, 1:] != pairs[0, :-1]
        image = torch.zeros(H * W, dtype=torch.int32, device=dev)
        image[pairs[0, first]] = (pairs[1, first] + 1).to(torch.int32)
        return image.view(H, W)

    def timed(fn, runs) -> dict:
        ms, peak, out = [], 0, None
        for r in range(runs + 1):                                     # run 0 warms up
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
        return {"ms_median": statistics.median(ms), "ms": ms, "peak_bytes_above_inputs": int(peak)}, out

    scenes = []
    for name in names:
        if name == "outlines_1m":
            from bench_outlines import segmentation
            xy_h, cell_h, n_cells = segmentation(10 ** 6, args.seed)
            rings = bd.cell_outlines(torch.from_numpy(xy_h).to(dev), torch.from_numpy(cell_h).to(dev), n_cells)
            o, v = rings["ring_offsets"], rings["xy"]
            shape, scale, translation = (8192, 8192), (9.765625, 9.765625), (1e4, 1e4)
        else:
            o_h, v_h, shape, scale, translation = host[name]
            o, v = torch.from_numpy(o_h).to(dev), torch.from_numpy(np.ascontiguousarray(v_h)).to(dev)
        kw = dict(scale=scale, translation=translation)
        entry = {"scene": name, "polygons": int(o.numel()) - 1, "vertices": int(v.shape[0]), "shape": list(shape), "scale": list(scale),
                 "blocks": {}}
        runs, composition_runs = (min(args.runs, c) for c in RUN_CAPS.get(name, (args.runs, args.composition_runs)))
        composition_runs = min(composition_runs, args.composition_runs)
        entry["runs"], entry["composition_runs"] = runs, composition_runs
        image = None
        for block in (1,) + BLOCKS:
            t, out = timed(lambda: rm.rasterize_rings(o, v, shape, _block=block, **kw), runs)
            c = dict(zip(rm.COUNTER_NAMES, out["counters"].tolist()))
            t["pixels_set_per_s"] = c["n_pixels_set"] / (t["ms_median"] * 1e-3)
            t["n_blocks_filled"] = c["n_blocks_filled"]
            entry["blocks"][str(block)] = t
            entry["counters"] = {k: c[k] for k in rm.COUNTER_NAMES[:6]}
            same = image is None or torch.equal(image, out["image"])
            entry["same_image_for_every_block"] = entry.get("same_image_for_every_block", True) and same
            image = out["image"]
            del out
            print(f"[rasterize] {name} block {block}: {t['ms_median']:.3f} ms", file=sys.stderr, flush=True)
        t, comp = timed(lambda: composition(o, v, shape, scale, translation), composition_runs)
        entry["composition"] = t
        entry["same_image_as_the_composition"] = bool(torch.equal(image, comp))
        del comp, image
        torch.cuda.empty_cache()
        best = min(BLOCKS, key=lambda b: entry["blocks"][str(b)]["ms_median"])
        entry["fastest_block"] = best
        entry["default_over_composition_time"] = entry["blocks"][str(rm.DEFAULT_BLOCK)]["ms_median"] / t["ms_median"]
        entry["default_over_block1_time"] = entry["blocks"][str(rm.DEFAULT_BLOCK)]["ms_median"] / entry["blocks"]["1"]["ms_median"]
        if args.cpu_polygons > 0:
            entry["cpu_oracle"] = cpu_oracle(o.cpu().numpy(), v.cpu().numpy(), shape, scale, translation, args.cpu_polygons, args.cpu_procs)
        scenes.append(entry)
        print(f"[rasterize] {name} " + " ".join(f"B{b}={entry['blocks'][str(b)]['ms_median']:.3f}ms" for b in (1,) + BLOCKS) +
              f" composition={t['ms_median']:.3f}ms same={entry['same_image_as_the_composition']} {entry['counters']}", file=sys.stderr, flush=True)
    total = {b: sum(s["blocks"][str(b)]["ms_median"] for s in scenes) for b in BLOCKS}
    res = {"what": "rasterize.rasterize_rings (predicate intersects, overlap lowest) against points_in_polygons over all pixel centres + "
                   "a scatter of the lowest polygon of every pixel",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "composition_runs": args.composition_runs, "run_caps": RUN_CAPS, "seed": args.seed,
           "timing": "device events around the whole Python call (host synchronisations included); median of the runs after one "
                     "warm-up; peak = torch's allocator peak above the inputs during one call",
           "default_block": rm.DEFAULT_BLOCK, "sum_of_medians_ms_by_block": total, "fastest_block_overall": min(total, key=total.get),
           "fastest_block_by_scene": {s["scene"]: s["fastest_block"] for s in scenes},
           "what_bounds_the_kernels": "not measured (no counter run was made)", "scenes": scenes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
