#!/usr/bin/env python
"""Time the adaptive tiling of a slide on the GPU: ``QuadTreeTiling`` (csrc/quadtree.hip) on ``--n`` float32 points whose
density differs by ``--contrast`` between the two halves of the slide, with ``--max-tile-size`` nodes per leaf.

Reports the median of ``--runs`` builds after ``--warmup`` (HIP events around the whole constructor: bounds, key pass,
radix sort, leaf work list, label pass, and the one read-back of the leaf count), the tile count and the min / median / max
tile population -- next to the populations a ``SquareTiling`` gets on the same points at the side ``fov.py`` derives from
the mean density -- and the bytes the build has to move, from which the achieved bandwidth follows.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def populations(counts: torch.Tensor) -> dict:
    c = counts[counts > 0].double()
    return {"tiles": int(c.numel()), "min": int(c.min()), "median": float(c.median()), "max": int(c.max()),
            "empty": int((counts == 0).sum())}


def timed(fn, runs: int, warmup: int):
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--max-tile-size", type=int, default=50_000)
    ap.add_argument("--contrast", type=float, default=10.0, help="density of the left half over the right half")
    ap.add_argument("--side-um", type=float, default=10.0 * math.sqrt(500_000), help="side of the slide")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quadtree.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd.tiles import QuadTreeTiling, SquareTiling

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(args.seed)
    L = float(args.side_um)
    pos = torch.rand(args.n, 2, generator=g, device=dev) * L
    dense = torch.rand(args.n, generator=g, device=dev) < args.contrast / (args.contrast + 1.0)
    pos[:, 0] = torch.where(dense, pos[:, 0] * 0.5, L * 0.5 + pos[:, 0] * 0.5)
    del dense
    torch.cuda.synchronize()

    tiling, build_ms = timed(lambda: QuadTreeTiling(pos, args.max_tile_size), args.runs, args.warmup)
    _, label_ms = timed(lambda: tiling.label(pos), args.runs, args.warmup)
    side = math.sqrt(args.max_tile_size / (args.n / (L * L)))            # what fov.py chooses from the mean density
    sq = SquareTiling(pos, side)
    sq_counts = torch.bincount(sq.label(pos), minlength=len(sq)).cpu()

    # bytes a build has to move, per point: the key pass reads 8 and writes 4; the radix sort reads the keys once for its
    # histograms and then reads and writes them once per 8-bit digit; the label pass reads 8 and writes 4
    key_bits = 2 * tiling.depth
    passes = -(-key_bits // 8)
    per_point = (8 + 4) + (4 + passes * 8) + (8 + 4)
    med = statistics.median(build_ms)
    res = {
        "what": "QuadTreeTiling build", "device": torch.cuda.get_device_name(0), "n_points": args.n,
        "max_tile_size": args.max_tile_size, "density_contrast": args.contrast, "slide_side_um": L,
        "depth": tiling.depth, "cell": tiling.cell, "key_bits": key_bits,
        "build_ms_median": med, "build_ms": build_ms, "runs": args.runs, "warmup": args.warmup,
        "label_ms_median": statistics.median(label_ms), "label_ms": label_ms,
        "quadtree": populations(tiling.counts), "over_max_tile_size": int((tiling.counts > args.max_tile_size).sum()),
        "square": {"side_um": side, **populations(sq_counts), "over_max_tile_size": int((sq_counts > args.max_tile_size).sum())},
        "bytes_per_point": per_point, "sort_passes_assumed": passes, "bytes_moved": per_point * args.n,
        "achieved_gb_per_s": per_point * args.n / (med * 1e-3) / 1e9,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
