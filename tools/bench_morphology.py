#!/usr/bin/env python
"""Time the boundary morphology features on the GPU: ``morphology.polygon_props`` (csrc/morphology.hip: one wave per
polygon; registers for rings of up to 64 vertices, LDS above) on synthetic star-shaped rings on slide coordinates,
already on the device.

Workloads: rings of 13 and of 25 vertices (Xenium's two fixed sizes) at ``--polygons`` polygons (default 10^5 and 10^6),
and a mix at each size of 99 % 13-vertex rings with 1 % rings of 200 .. 2000 vertices.  Per workload, after one warm-up,
``--runs`` calls of the C entry point are timed with device events and the median is reported: polygons per second,
milliseconds, the compulsory bytes per polygon (16 n for the vertices, 8 for the offset, 96 for the row of 12 float64) and
the fraction of 8 TB/s those bytes amount to at the measured rate.  For the mix, the polygons of each route are also
timed as batches of their own, which gives the share of time spent in each route.

The comparison figure is a CPU figure: the float64 numpy oracle of tests/morphology_cases.py (``props_f64``, one polygon
at a time) on 10^5 13-vertex rings over ``--cpu-procs`` processes (default 16), run before the GPU is touched.

One JSON line; ``--out`` also writes it to a file (profiles/morphology_polygons_per_s.json is the committed measurement).
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

SLIDE = (73211.25, 48907.5)
HBM_BYTES_PER_S = 8e12


def star_rings(n_polygons: int, n_vertices: int, seed: int) -> np.ndarray:
    """[P, n, 2] float64: random star-shaped rings of ~10 across on slide coordinates"""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, 2 * np.pi, (n_polygons, n_vertices)), axis=1)
    r = rng.uniform(3.0, 7.0, (n_polygons, 1)) * rng.uniform(0.6, 1.0, (n_polygons, n_vertices))
    centre = np.asarray(SLIDE) + rng.uniform(-5000.0, 5000.0, (n_polygons, 1, 2))
    return centre + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=2)


def mixed(n_polygons: int, seed: int):
    """(ring_offsets, xy, is_long): 99 % 13-vertex rings, 1 % rings of 200 .. 2000 vertices"""
    rng = np.random.default_rng(seed)
    counts = np.full(n_polygons, 13, dtype=np.int64)
    long_ids = rng.choice(n_polygons, max(n_polygons // 100, 1), replace=False)
    counts[long_ids] = rng.integers(200, 2001, long_ids.size)
    offsets = np.zeros(n_polygons + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(counts)
    owner = np.repeat(np.arange(n_polygons), counts)
    k = np.arange(offsets[-1]) - offsets[owner]
    ang = 2 * np.pi * (k + rng.uniform(0.0, 0.9, k.size)) / counts[owner]
    r = rng.uniform(3.0, 7.0, n_polygons)[owner] * rng.uniform(0.6, 1.0, k.size)
    centre = np.asarray(SLIDE) + rng.uniform(-5000.0, 5000.0, (n_polygons, 2))
    return offsets, centre[owner] + np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1), counts > 64


def _oracle_chunk(rings: np.ndarray) -> float:
    import morphology_cases as mc
    return sum(mc.props_f64(r)["area"] for r in rings)


def cpu_oracle_rate(n_polygons: int, procs: int) -> dict:
    rings = star_rings(n_polygons, 13, 1)
    chunks = np.array_split(rings, procs * 8)
    with multiprocessing.get_context("fork").Pool(procs) as pool:
        pool.map(_oracle_chunk, chunks[:procs])                       # start the workers, import numpy
        t = time.perf_counter()
        pool.map(_oracle_chunk, chunks)
        dt = time.perf_counter() - t
    return {"what": "CPU figure: numpy float64 oracle (tests/morphology_cases.props_f64), one polygon at a time",
            "processes": procs, "polygons": n_polygons, "vertices": 13, "seconds": dt, "polygons_per_s": n_polygons / dt}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--polygons", default="100000,1000000", help="polygon counts, comma separated")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--cpu-polygons", type=int, default=100000, help="0 skips the CPU figure")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    cpu = cpu_oracle_rate(args.cpu_polygons, args.cpu_procs) if args.cpu_polygons > 0 else None
    print(f"[morphology] {cpu}", file=sys.stderr, flush=True)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_morphology.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import _lib as L
    dev = torch.device("cuda:0")

    def timed(offsets: np.ndarray, xy: np.ndarray) -> dict:
        o, v = torch.from_numpy(offsets).to(dev), torch.from_numpy(np.ascontiguousarray(xy)).to(dev)
        P, V = int(o.numel()) - 1, int(v.shape[0])
        props = torch.empty(P, L.MORPH_COLS, dtype=torch.float64, device=dev)
        ws, ws_bytes = L.workspace("segger_morphology_workspace_bytes", dev, P)
        ms = []
        for r in range(args.runs + 1):                                # run 0 warms up
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            L.call("segger_polygon_props", dev, o.data_ptr(), v.data_ptr(), P, V, props.data_ptr(), ws.data_ptr(), ws_bytes)
            stop.record()
            stop.synchronize()
            if r:
                ms.append(start.elapsed_time(stop))
        words = ws[:12].view(torch.int32).tolist()
        assert words[0] == 0 and words[1] + words[2] == P and bool(torch.isfinite(props).all())
        med = statistics.median(ms)
        bytes_per_polygon = 16.0 * V / P + 8 + 96
        rate = P / (med * 1e-3)
        return {"polygons": P, "vertices": V, "register_route": words[1], "lds_route": words[2], "ms_median": med, "ms": ms,
                "polygons_per_s": rate, "compulsory_bytes_per_polygon": bytes_per_polygon,
                "fraction_of_8TBps": rate * bytes_per_polygon / HBM_BYTES_PER_S}

    workloads = []
    for P in [int(s) for s in args.polygons.split(",") if s]:
        for n in (13, 25):
            entry = {"workload": f"star{n}", **timed(np.arange(P + 1, dtype=np.int64) * n, star_rings(P, n, args.seed).reshape(-1, 2))}
            workloads.append(entry)
            print(f"[morphology] {entry}", file=sys.stderr, flush=True)
        offsets, xy, is_long = mixed(P, args.seed)
        entry = {"workload": "mix 99 % star13 + 1 % of 200 .. 2000 vertices", **timed(offsets, xy)}
        counts = np.diff(offsets)
        for name, pick in (("lds_route_alone", is_long), ("register_route_alone", ~is_long)):
            keep = np.repeat(pick, counts)
            sub = np.zeros(int(pick.sum()) + 1, dtype=np.int64)
            sub[1:] = np.cumsum(counts[pick])
            entry[name] = {k: v for k, v in timed(sub, xy[keep]).items() if k in ("polygons", "vertices", "ms_median")}
        both = entry["lds_route_alone"]["ms_median"] + entry["register_route_alone"]["ms_median"]
        entry["share_of_time"] = {"lds_route": entry["lds_route_alone"]["ms_median"] / both,
                                  "register_route": entry["register_route_alone"]["ms_median"] / both}
        workloads.append(entry)
        print(f"[morphology] {entry}", file=sys.stderr, flush=True)
    res = {"what": "segger_polygon_props (binning + register route + LDS route) on synthetic star-shaped rings on slide coordinates",
           "device": torch.cuda.get_device_name(0), "runs": args.runs, "seed": args.seed,
           "timing": "device events around the three launches of one call; median of the runs after one warm-up",
           "cpu_comparison": cpu, "workloads": workloads}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
