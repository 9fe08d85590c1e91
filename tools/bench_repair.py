"""Throughput of segger_amd.repair_rings / resort_rings -> profiles/repair_rings_per_s.json, one JSON line per leg.

Legs: (i) repair_rings on 10^6 valid 13-vertex rings (Xenium's fixed-length boundaries) -- the price of the check alone,
beside rings_simple alone on the same input; (ii) the same input with 1 % of the rings scrambled; (iii) the contours of the
Voronoi label image of tools/bench_contours.py, every ring scrambled: resort_rings on both LDS tiers and repair_rings.
Timed: the entry point with device events after a warm-up, median of 20 calls with the range (the wrappers' waits for the
device included).  The CPU figure is the reference's formula -- np.argsort(np.arctan2(...)) around the mean of the closed
sequence, per ring -- on 16 processes over a SUBSAMPLE of the scrambled rings, scaled to the leg by ring count and labelled
as such; it sorts only, it does not check validity.  The reference's own shapely loop (is_valid, resort, is_valid) cannot be
run here: no figure for it.

    python tools/bench_repair.py [--size 4096] [--rings 1000000] [--out profiles/repair_rings_per_s.json]"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_simplify import timed  # noqa: E402


def fixed_rings(n_rings, n_verts, dev, seed=0):
    """valid counter-clockwise rings of n_verts integer vertices each, star-shaped around their own centre"""
    g = torch.Generator(device=dev).manual_seed(seed)
    k = torch.arange(n_verts, device=dev, dtype=torch.float64)[None, :]
    ang = (k + 0.6 * torch.rand(n_rings, n_verts, generator=g, device=dev, dtype=torch.float64)) / n_verts * (2 * torch.pi)
    rad = 60.0 * (0.8 + 0.2 * torch.rand(n_rings, n_verts, generator=g, device=dev, dtype=torch.float64))
    p = torch.arange(n_rings, device=dev)
    cx, cy = (p % 1000 * 200.0)[:, None], (p // 1000 * 200.0)[:, None]
    xy = torch.stack([torch.round(rad * torch.cos(ang)) + cx, torch.round(rad * torch.sin(ang)) + cy], 2)
    off = torch.arange(n_rings + 1, device=dev, dtype=torch.int64) * n_verts
    return off, xy


def scramble(off, xy, which, seed=1):
    """the vertices of the rings `which` (bool [P]) in a random order, the other rings as they are"""
    dev = xy.device
    counts = off[1:] - off[:-1]
    ring_of = torch.repeat_interleave(torch.arange(counts.numel(), device=dev), counts)
    g = torch.Generator(device=dev).manual_seed(seed)
    within = torch.arange(xy.shape[0], device=dev) - off[ring_of]
    key = torch.where(which[ring_of], torch.rand(xy.shape[0], generator=g, device=dev, dtype=torch.float64),
                      within.double() / (counts[ring_of].double() + 1.0))
    return xy[torch.argsort(ring_of.double() + key)].contiguous()


def _numpy_chunk(rings):
    import numpy as np
    t0 = time.perf_counter()
    for r in rings:
        closed = np.vstack([r, r[:1]])
        c = closed.mean(axis=0)
        closed[np.argsort(np.arctan2(closed[:, 1] - c[1], closed[:, 0] - c[0]))]
    return time.perf_counter() - t0


def cpu_seconds(off, xy, which, n_sub=1024):
    ids = which.nonzero().reshape(-1)
    pick = ids[torch.linspace(0, ids.numel() - 1, min(n_sub, ids.numel())).long()].tolist()
    o = off.cpu()
    rings = [xy[int(o[p]):int(o[p + 1])].cpu().numpy() for p in pick]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(16) as pool:
        pool.map(_numpy_chunk, [rings[c::16] for c in range(16)])
    wall = time.perf_counter() - t0
    return {"subsample_rings": len(rings), "processes": 16, "subsample_wall_s": wall, "rings_to_sort": int(ids.numel()),
            "scaled_to_leg_s": wall * ids.numel() / len(rings), "scaled": True,
            "what": "np.argsort(np.arctan2) around the closed ring's mean, the sort only, pool start-up included; not shapely"}


def leg(name, off, xy, which, no_cpu, tiers=False):
    from segger_amd import repair_rings, resort_rings, rings_simple
    P = off.numel() - 1
    out = repair_rings(off, xy, on_failure="keep")
    row = {"leg": name, "rings": P, "vertices": int(xy.shape[0]), **dict(zip(("n_invalid_in", "n_resorted", "n_still_invalid"),
                                                                             out["counters"].tolist())),
           "repair_rings": timed(lambda: repair_rings(off, xy, on_failure="keep")), "rings_simple_alone": timed(lambda: rings_simple(off, xy)),
           "timer": "device events around the Python entry point"}
    row["rings_per_s"] = P / row["repair_rings"]["median_s"]
    if which is not None:
        sel = ~rings_simple(off, xy)[0]
        row["resort_rings_of_the_invalid"] = timed(lambda: resort_rings(off, xy, sel))
        if tiers:
            row["resort_rings_all_small_tier_where_it_fits"] = timed(lambda: resort_rings(off, xy))
            row["resort_rings_all_large_tier_only"] = timed(lambda: resort_rings(off, xy, _route="large"))
            row["longest_ring"] = int((off[1:] - off[:-1]).max())
        if not no_cpu:
            row["cpu_numpy"] = cpu_seconds(off, xy, which)
    row["lds_counters"] = "not measured (no counter run was made)"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--labels", type=int, default=5000)
    ap.add_argument("--rings", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repair_rings_per_s.json"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from bench_contours import voronoi_scene
    from segger_amd import label_contours
    dev = torch.device("cuda:0")
    rows = []
    off, xy3 = fixed_rings(args.rings, 13, dev)
    xy = xy3.reshape(-1, 2).contiguous()
    rows.append(leg(f"(i) {args.rings} valid 13-vertex rings", off, xy, None, args.no_cpu))
    print(json.dumps(rows[-1]), flush=True)
    which = torch.arange(args.rings, device=dev) % 100 == 7
    rows.append(leg(f"(ii) {args.rings} 13-vertex rings, 1 % scrambled", off, scramble(off, xy, which), which, args.no_cpu))
    print(json.dumps(rows[-1]), flush=True)
    del xy, xy3
    c = label_contours(voronoi_scene(args.size, args.labels, 0, dev))
    which = torch.ones(c["ring_offsets"].numel() - 1, dtype=torch.bool, device=dev)
    rows.append(leg(f"(iii) voronoi {args.size}x{args.size}, {args.labels} labels, every contour scrambled", c["ring_offsets"],
                    scramble(c["ring_offsets"], c["xy"], which), which, args.no_cpu, tiers=True))
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
