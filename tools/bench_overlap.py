"""Throughput of segger_amd.polygon_overlaps -> profiles/overlap_pairs_per_s.json, one JSON line per scene.

Scenes: (a) cell_outlines rings of n cells against 13-vertex rings round the same cells' centres, n = 5 10^3 and 5 10^4;
(b) the Voronoi label image of tools/bench_contours.py through label_contours, unsimplified against simplify_rings at the
reference's tolerance; (c) one pair of 4096-vertex rings alone, 1.7 10^7 edge pairs on one wave.  Timed: the entry point with
device events after a warm-up, median of 20 calls (the wrapper's five waits for the device included); the candidate stage is
timed on its own C entry point the same way.  The CPU figure is the float64 numpy formula of tests/overlap_cases.py on 16
processes over a SUBSAMPLE of the intersecting pairs, scaled to the scene by pair count and labelled as such.  Shapely's
sjoin and intersection (the reference's) cannot be run here: no figure for them.  Nothing here says what bounds the pair kernel.

    python tools/bench_overlap.py [--cells 5000 50000] [--out profiles/overlap_pairs_per_s.json]"""
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


def cells_scene(n_cells, dev, per_cell=40, seed=0):
    """transcripts of n_cells cells on a square lattice of pitch 30, blobs of radius ~14 -> (cell_outlines rings, 13-gons)"""
    from segger_amd import cell_outlines
    g = torch.Generator(device=dev).manual_seed(seed)
    side = int(n_cells ** 0.5) + 1
    cell = torch.arange(n_cells, device=dev).repeat_interleave(per_cell)
    centre = torch.stack([(cell % side) * 30.0, (cell // side) * 30.0], 1).double()
    xy = centre + torch.randn(cell.numel(), 2, generator=g, device=dev, dtype=torch.float64) * 7.0
    out = cell_outlines(xy, cell.int(), n_cells)
    ang = torch.arange(13, device=dev, dtype=torch.float64) * (2 * torch.pi / 13)
    c = centre[::per_cell] + torch.randn(n_cells, 2, generator=g, device=dev, dtype=torch.float64) * 4.0
    ring = c[:, None, :] + 13.0 * torch.stack([torch.cos(ang), torch.sin(ang)], 1)[None]
    off_b = torch.arange(n_cells + 1, device=dev, dtype=torch.int64) * 13
    return out["ring_offsets"], out["xy"], off_b, ring.reshape(-1, 2).contiguous()


def _oracle_chunk(pairs):
    import overlap_cases as oc
    t0 = time.perf_counter()
    for a, b in pairs:
        oc.area_formula_f64(a, b)
    return time.perf_counter() - t0


def cpu_oracle_seconds(sets, pairs, n_sub=512):
    E = pairs.shape[1]
    pick = torch.linspace(0, E - 1, min(n_sub, E)).long()
    off_a, xy_a, off_b, xy_b = (t.cpu() for t in sets)
    work = [(xy_a[int(off_a[a]):int(off_a[a + 1])].numpy(), xy_b[int(off_b[b]):int(off_b[b + 1])].numpy())
            for a, b in pairs[:, pick].T.tolist()]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(16) as pool:
        pool.map(_oracle_chunk, [work[c::16] for c in range(16)])
    wall = time.perf_counter() - t0
    return {"subsample_pairs": len(work), "processes": 16, "subsample_wall_s": wall, "scaled_to_scene_s": wall * E / len(work), "scaled": True,
            "what": "the float64 numpy formula of tests/overlap_cases.py on the intersecting pairs only, pool start-up included; not shapely"}


def candidate_stage(sets):
    """the candidate entry point alone, with the grid polygon_overlaps would choose at its default"""
    from segger_amd import _lib as L
    off_a, xy_a, off_b, xy_b = sets
    n_a, n_b = off_a.numel() - 1, off_b.numel() - 1
    lo = torch.minimum(xy_a.min(0).values, xy_b.min(0).values).tolist()
    hi = torch.maximum(xy_a.max(0).values, xy_b.max(0).values).tolist()
    w, h = max(hi[0] - lo[0], 1e-6), max(hi[1] - lo[1], 1e-6)
    cell = max((w * h / max(n_a, n_b)) ** 0.5, max(w, h) / 30000.0)
    nx, ny = int(w / cell) + 1, int(h / cell) + 1
    ws, ws_bytes = L.workspace("segger_polygon_overlap_workspace_bytes", xy_a.device, n_a, n_b, nx, ny)
    total = torch.zeros(1, dtype=torch.int64, device=xy_a.device)
    return timed(lambda: L.call("segger_polygon_overlap_candidates", xy_a.device, off_a.data_ptr(), xy_a.data_ptr(), n_a, xy_a.shape[0],
                                off_b.data_ptr(), xy_b.data_ptr(), n_b, xy_b.shape[0], lo[0], lo[1], cell, nx, ny, total.data_ptr(),
                                ws.data_ptr(), ws_bytes))


def scene_row(name, sets, no_cpu):
    from segger_amd import match_polygons, polygon_overlaps
    out = polygon_overlaps(*sets)
    c = dict(zip(("candidates", "intersecting", "lds_pairs", "wide"), out["counters"].tolist()))
    t = timed(lambda: polygon_overlaps(*sets))
    tc = candidate_stage(sets)
    row = {"scene": name, "polygons_a": sets[0].numel() - 1, "polygons_b": sets[2].numel() - 1, "vertices_a": sets[1].shape[0],
           "vertices_b": sets[3].shape[0], **c, "overlaps": t, "candidate_pairs_per_s": c["candidates"] / t["median_s"],
           "intersecting_pairs_per_s": c["intersecting"] / t["median_s"], "candidate_stage": tc,
           "candidate_stage_share": tc["median_s"] / t["median_s"], "match_polygons": timed(lambda: match_polygons(out)),
           "timer": "device events around the Python entry point"}
    if not no_cpu and c["intersecting"]:
        row["cpu_oracle"] = cpu_oracle_seconds(sets, out["pairs"].cpu())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="*", default=[5000, 50000])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--labels", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_pairs_per_s.json"))
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import overlap_cases as oc
    from bench_contours import voronoi_scene
    from segger_amd import contour_tolerance, label_contours, simplify_rings
    dev = torch.device("cuda:0")
    rows = []
    for n in args.cells:
        rows.append(scene_row(f"(a) {n} cell_outlines rings against {n} 13-vertex rings", cells_scene(n, dev), args.no_cpu))
        print(json.dumps(rows[-1]), flush=True)
    c = label_contours(voronoi_scene(args.size, args.labels, 0, dev))
    s = simplify_rings(c["ring_offsets"], c["xy"], contour_tolerance(c["ring_offsets"], c["xy"]))
    rows.append(scene_row(f"(b) voronoi {args.size}x{args.size}, {args.labels} labels: contours against their simplification",
                          (c["ring_offsets"], c["xy"], s["ring_offsets"], s["xy"]), args.no_cpu))
    print(json.dumps(rows[-1]), flush=True)
    a = oc.star(oc.MAX_VERTS, 77, scale=1 << 20)
    pair = tuple(torch.from_numpy(t).to(dev) for t in oc.csr([a]) + oc.csr([a[::-1].copy() + 1000.0]))
    rows.append(scene_row("(c) one pair of 4096-vertex rings", pair, args.no_cpu))
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
