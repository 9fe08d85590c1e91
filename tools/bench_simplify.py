"""Throughput of segger_amd.simplify_rings -> profiles/simplify_rings_per_s.json, one JSON line per scene.

Scenes: the Voronoi label image of tools/bench_contours.py put through label_contours, then simplify_rings at the reference's
tolerance (contour_tolerance, sqrt(area).mean() / 50); and a synthetic batch of 10^6 ragged star rings of ~100 integer
vertices at tolerance 2.  Timed: the entry point with device events after a warm-up, median of 20 calls with the range (the
wrapper's two waits for the device included).  Also: morphology_features and points_in_polygons on the rings before and
after the simplification -- the reason the step exists -- each the median of 20; rings_simple once per scene.  The CPU
figure is the numpy oracle of tests/simplify_cases.py on 16 processes over a SUBSAMPLE of the rings, scaled to the scene
by ring count and labelled as such.  Shapely's own loop (the reference's) cannot be run here: no figure for it.

    python tools/bench_simplify.py [--size 4096] [--rings 1000000] [--out profiles/simplify_rings_per_s.json]"""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = 20


def timed(fn, calls=CALLS):
    fn()                                                             # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "calls": calls}


def star_batch(n_rings, dev, seed=0):
    """ragged star rings of 68 .. 132 integer vertices, on the device"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    counts = torch.randint(68, 133, (n_rings,), generator=gen).to(dev)
    off = torch.zeros(n_rings + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=off[1:])
    V = int(off[-1])
    ring_of = torch.repeat_interleave(torch.arange(n_rings, device=dev), counts)
    k = torch.arange(V, device=dev) - off[ring_of]
    g = torch.Generator(device=dev).manual_seed(seed)
    ang = (k + 0.8 * torch.rand(V, generator=g, device=dev, dtype=torch.float64)) / counts[ring_of] * (2 * torch.pi)
    rad = 60.0 * (0.6 + 0.4 * torch.rand(V, generator=g, device=dev, dtype=torch.float64))
    centre = (ring_of % 1000 * 200.0, ring_of // 1000 * 200.0)
    xy = torch.stack([torch.round(rad * torch.cos(ang)) + centre[0], torch.round(rad * torch.sin(ang)) + centre[1]], 1)
    return off, xy.contiguous()


def _oracle_chunk(args):
    import simplify_cases as sc
    rings, tol = args
    t0 = time.perf_counter()
    for r in rings:
        sc.simplify_ring(r, tol)
    return time.perf_counter() - t0


def cpu_oracle_seconds(off, xy, tol, n_sub=1024):
    P = off.numel() - 1
    pick = torch.linspace(0, P - 1, min(n_sub, P)).long().tolist()
    o = off.cpu()
    rings = [xy[int(o[p]):int(o[p + 1])].cpu().numpy() for p in pick]
    chunks = [(rings[c::16], tol) for c in range(16)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(16) as pool:
        pool.map(_oracle_chunk, chunks)
    wall = time.perf_counter() - t0
    return {"subsample_rings": len(rings), "processes": 16, "subsample_wall_s": wall, "scaled_to_scene_s": wall * P / len(rings),
            "scaled": True, "what": "the numpy oracle of tests/simplify_cases.py, pool start-up included; not shapely"}


def scene_row(name, off, xy, tol, points, no_cpu):
    from segger_amd import morphology_features, points_in_polygons, rings_simple, simplify_rings
    P = off.numel() - 1
    s = simplify_rings(off, xy, tol)
    c = dict(zip(("vertices_in", "vertices_out", "sections", "refused", "passed_through", "restored", "longest_out"),
                 s["counters"].tolist()))
    t = timed(lambda: simplify_rings(off, xy, tol))
    row = {"scene": name, "rings": P, "tolerance": float(tol), **c, "simplify": t, "rings_per_s": P / t["median_s"],
           "vertices_in_per_s": c["vertices_in"] / t["median_s"], "timer": "device events around the Python entry point"}
    row["large_tier_only"] = timed(lambda: simplify_rings(off, xy, tol, _route="large"), 5) if P <= 100000 else "not measured"
    row["morphology_features_before"] = timed(lambda: morphology_features(off, xy))
    row["morphology_features_after"] = timed(lambda: morphology_features(s["ring_offsets"], s["xy"]))
    if points is not None:
        row["points"] = int(points.shape[0])
        row["points_in_polygons_before"] = timed(lambda: points_in_polygons(points, off, xy))
        row["points_in_polygons_after"] = timed(lambda: points_in_polygons(points, s["ring_offsets"], s["xy"]))
    else:
        row["points_in_polygons_before"] = row["points_in_polygons_after"] = "not measured"
    row["rings_simple_before"] = timed(lambda: rings_simple(off, xy), 5)
    ok_in, ok_out = rings_simple(off, xy)[0], rings_simple(s["ring_offsets"], s["xy"])[0]
    row["simple_in"], row["simple_out"], row["simple_in_not_out"] = int(ok_in.sum()), int(ok_out.sum()), int((ok_in & ~ok_out).sum())
    if not no_cpu:
        row["cpu_oracle"] = cpu_oracle_seconds(off, xy, float(tol))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--labels", type=int, default=5000)
    ap.add_argument("--rings", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_rings_per_s.json"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from bench_contours import voronoi_scene
    from segger_amd import contour_tolerance, label_contours
    dev = torch.device("cuda:0")
    lines = []
    img = voronoi_scene(args.size, args.labels, 0, dev)
    c = label_contours(img)
    tol = contour_tolerance(c["ring_offsets"], c["xy"])
    pts = torch.rand(1000000, 2, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * args.size
    rows = [scene_row(f"voronoi {args.size}x{args.size}, {args.labels} labels, contour_tolerance", c["ring_offsets"], c["xy"], tol, pts,
                      args.no_cpu)]
    del img, c
    off, xy = star_batch(args.rings, dev)
    rows.append(scene_row(f"{args.rings} ragged stars of ~100 vertices, tolerance 2", off, xy, 2.0, None, args.no_cpu))
    for row in rows:
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
