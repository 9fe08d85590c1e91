"""Throughput of segger_amd.label_contours on synthetic Voronoi label images with a background gap ->
profiles/contours_pixels_per_s.json, one JSON line per scene.

Timed: the entry point with device events, median of 20 calls (the wrapper's two waits for the device included).  The
kernels' own times come from one profiled call (torch.profiler's device activity): pass A (ct_scan_kernel) and the
per-label passes (ct_trace_kernel, ct_offsets_kernel, ct_emit_kernel) separately; "not measured" when the profiler gives no
device times.  Pass A is also given as a fraction of the 8 TB/s floor for its compulsory bytes (4 B per pixel, + 1 with a
compartment plane).  The CPU figure is the numpy oracle of tests/contour_cases.py on 16 processes over a SUBSAMPLE (a
512 x 512 corner cut into 16 tiles, labels cut at the tile edges), scaled to the scene by pixel count and labelled as such.

    python tools/bench_contours.py [--size 4096] [--out profiles/contours_pixels_per_s.json]"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8e12


def voronoi_scene(size, n_labels, seed, dev):
    """a jittered-grid Voronoi label image on the device: a pixel takes the nearest of the seeds of its 3 x 3 grid cells,
    background where that seed is farther than 0.42 of the grid pitch"""
    g = int(round(n_labels ** 0.5))
    pitch = size / g
    gen = torch.Generator(device="cpu").manual_seed(seed)
    sx = ((torch.arange(g)[None, :] + torch.rand(g, g, generator=gen)) * pitch).to(dev)
    sy = ((torch.arange(g)[:, None] + torch.rand(g, g, generator=gen)) * pitch).to(dev)
    out = torch.zeros(size, size, dtype=torch.int32, device=dev)
    rows = 256
    for y0 in range(0, size, rows):
        yy = torch.arange(y0, min(y0 + rows, size), device=dev, dtype=torch.float32)[:, None].expand(-1, size)
        xx = torch.arange(size, device=dev, dtype=torch.float32)[None, :].expand(yy.shape[0], -1)
        cy, cx = (yy / pitch).long().clamp(0, g - 1), (xx / pitch).long().clamp(0, g - 1)
        best = torch.full(yy.shape, float("inf"), device=dev)
        lab = torch.zeros(yy.shape, dtype=torch.int64, device=dev)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ny, nx = (cy + dy).clamp(0, g - 1), (cx + dx).clamp(0, g - 1)
                d2 = (xx - sx[ny, nx]) ** 2 + (yy - sy[ny, nx]) ** 2
                take = d2 < best
                best = torch.where(take, d2, best)
                lab = torch.where(take, ny * g + nx + 1, lab)
        out[y0:y0 + yy.shape[0]] = torch.where(best > (0.42 * pitch) ** 2, 0, lab).to(torch.int32)
    return out


def _oracle_tile(tile):
    import contour_cases as cc
    t0 = time.perf_counter()
    n = len(cc.label_rings(tile))
    return time.perf_counter() - t0, n


def cpu_oracle_seconds(img, size):
    sub = img[:512, :512].cpu().numpy()
    tiles = [sub[y:y + 128, x:x + 128].copy() for y in range(0, 512, 128) for x in range(0, 512, 128)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(16) as pool:
        res = pool.map(_oracle_tile, tiles)
    wall = time.perf_counter() - t0
    return {"subsample": "512 x 512 corner as 16 tiles of 128 x 128, labels cut at the tile edges", "processes": 16,
            "subsample_wall_s": wall, "subsample_labels": int(sum(n for _, n in res)),
            "scaled_to_scene_s": wall * (size * size) / (512 * 512), "scaled": True}


def kernel_times(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        t = {}
        for e in prof.key_averages():
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0)
            for k in ("ct_scan_kernel", "ct_trace_kernel", "ct_offsets_kernel", "ct_emit_kernel"):
                if k in e.key and us:
                    t[k] = t.get(k, 0.0) + us * 1e-6
        return t or None
    except Exception:                                                # no device activity from the profiler here
        return None


def bench(size, n_labels, with_comp, dev):
    from segger_amd import label_contours
    img = voronoi_scene(size, n_labels, 0, dev)
    comp = codes = None
    if with_comp:
        comp, codes = torch.ones(size, size, dtype=torch.uint8, device=dev), (1, 2)
    out = label_contours(img, comp, codes)
    c = out["counters"].tolist()
    times = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        label_contours(img, comp, codes)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    med = statistics.median(times)
    kt = kernel_times(lambda: label_contours(img, comp, codes))
    floor = size * size * (5 if with_comp else 4) / HBM_BYTES_PER_S
    row = {"scene": f"voronoi {size}x{size}", "compartment_plane": with_comp, "labels_present": c[0], "labels_kept": c[1],
           "vertices": c[2], "borders": c[4], "longest_ring": c[5], "labels_on_global_route": c[9],
           "entry_point_median_s": med, "entry_point_min_s": min(times), "pixels_per_s": size * size / med,
           "labels_per_s": c[0] / med, "calls": 20, "timer": "device events around the Python entry point"}
    if kt and "ct_scan_kernel" in kt:
        per_label = sum(v for k, v in kt.items() if k != "ct_scan_kernel")
        row.update({"pass_a_s": kt["ct_scan_kernel"], "per_label_passes_s": per_label, "kernels_s": kt,
                    "pass_a_floor_s": floor, "pass_a_fraction_of_8TBps_floor": floor / kt["ct_scan_kernel"],
                    "kernel_timer": "torch.profiler device activity, one call"})
    else:
        row.update({"pass_a_s": "not measured", "per_label_passes_s": "not measured", "pass_a_floor_s": floor})
    row["per_label_pass_bound"] = "not measured (no counter run was made)"
    return row, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours_pixels_per_s.json"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for n_labels, with_comp in ((5000, False), (20000, False), (20000, True)):
        row, img = bench(args.size, n_labels, with_comp, dev)
        if not args.no_cpu and not with_comp:
            row["cpu_oracle"] = cpu_oracle_seconds(img, args.size)
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
