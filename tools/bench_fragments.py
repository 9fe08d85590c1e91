"""Times segger_amd.fragments on synthetic tiles and writes profiles/fragments_edges_per_s.json.

Scenes: transcripts on a jittered square lattice, each with k neighbours drawn from fixed offsets of its 5 x 5 neighbourhood
(a kNN-shaped, spatially local directed graph), about 30 % unassigned at random, unit-norm fp32 embeddings of C = 64 that
agree inside 8 x 8 blocks and disagree across them.  1e6 transcripts / 1.5e7 edges and 1e7 / 1.5e8 at k = 15, and one scene
on the reference's default graph shape (k = 5; every lattice neighbour lies within its max_dist = 5).

Timed by device events around the entry points (``update``: one launch; ``result``: finalize and its one wait), the median
of ``--reps`` with min and max.  The baseline is the obvious alternative on the same inputs: boolean filter of the live
edges, gather and ``torch.cosine_similarity`` on the device, then ``scipy.sparse.csgraph.connected_components`` on the host,
transfer included (wall clock; fewer repetitions, it is slow).  Nothing here is a counter run: what bounds the kernel is
not measured."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OFFSETS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1), (2, 0), (-2, 0), (0, 2), (0, -2), (2, 1), (-2, -1), (1, 2)]


def scene(n, k, C, dev, seed=0):
    side = int(np.ceil(np.sqrt(n)))
    g = torch.Generator(device=dev).manual_seed(seed)
    i = torch.arange(n, device=dev)
    x, y = i % side, i // side
    src, dst = [], []
    for dx, dy in OFFSETS[:k]:
        xx, yy = (x + dx).clamp(0, side - 1), (y + dy).clamp(0, side - 1)
        j = (yy * side + xx).clamp(max=n - 1)
        src.append(i)
        dst.append(j)
    ei = torch.stack([torch.stack(src, 1).view(-1), torch.stack(dst, 1).view(-1)])        # grouped by source, like a kNN table
    cls = ((x // 8) * 7 + (y // 8) * 3) % 16
    z = 0.04 * torch.randn(n, C, device=dev, generator=g)
    z[i, cls] += 1.0
    z = torch.nn.functional.normalize(z, dim=1)
    un = torch.rand(n, device=dev, generator=g) < 0.3
    return z, ei, un


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed(fn, reps, before=None):
    out, ms = None, []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, stats(ms)


def baseline(z, ei, un, thr, min_size):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    s, d = ei
    live = un[s] & un[d] & (s != d)
    s, d = s[live], d[live]
    keep = torch.cosine_similarity(z[s], z[d], dim=1) >= thr
    s, d = s[keep].cpu().numpy(), d[keep].cpu().numpy()
    n = z.shape[0]
    _, lab = connected_components(coo_matrix((np.ones(s.size, np.int8), (s, d)), shape=(n, n)), directed=False)
    unn = un.cpu().numpy()
    size = np.bincount(lab[unn], minlength=lab.max() + 1)
    n_frag = int((size >= min_size).sum())
    labels = torch.from_numpy(lab).to(z.device)
    torch.cuda.synchronize()
    return n_frag, (time.perf_counter() - t0) * 1e3


def run(name, n, k, C, reps, base_reps, dev):
    from segger_amd import FragmentAccumulator
    z, ei, un = scene(n, k, C, dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()
    acc = FragmentAccumulator(n, un, 0.5, dev)
    acc.update(z, ei)
    res = acc.result(5)                                                  # warm-up, and the shares
    peak = torch.cuda.max_memory_allocated() - held
    _, t_up = timed(lambda: acc.update(z, ei), reps, before=acc.reset)
    _, t_fin = timed(lambda: acc.result(5), reps, before=lambda: (acc.reset(), acc.update(z, ei)))    # a forest not yet flattened
    base = [baseline(z, ei, un, 0.5, 5) for _ in range(base_reps)]
    assert base[0][0] == res["n_fragments"], (base[0][0], res["n_fragments"])
    t_base = stats([b[1] for b in base])
    e = int(ei.shape[1])
    ours = t_up["median_ms"] + t_fin["median_ms"]
    gather = res["n_live_edges"] * 2 * C * z.element_size()
    row = {"scene": name, "n_transcripts": n, "n_edges": e, "k": k, "channels": C, "dtype": "float32",
           "unassigned_share": res["n_candidates"] / n, "live_share": res["n_live_edges"] / e,
           "kept_share_of_live": res["n_kept_edges"] / max(res["n_live_edges"], 1), "n_components": res["n_components"],
           "n_fragments": res["n_fragments"], "update": t_up, "result": t_fin, "baseline_torch_scipy": t_base,
           "baseline_over_ours": t_base["median_ms"] / ours, "edges_per_s_update": e / (t_up["median_ms"] * 1e-3),
           "stage_b_gather_bytes": gather, "stage_b_bytes_per_s_over_the_whole_update": gather / (t_up["median_ms"] * 1e-3),
           "stage_b_share_of_8TBps": gather / (t_up["median_ms"] * 1e-3) / 8e12,
           "peak_bytes_above_inputs": int(peak), "what_bounds_the_kernel": "not measured (no counter run)"}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--large", action="store_true", help="also the 1e7-transcript scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fragments_edges_per_s.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [run("tile_1e6_k15", 1_000_000, 15, 64, a.reps, 5, dev), run("reference_shape_1e6_k5", 1_000_000, 5, 64, a.reps, 5, dev)]
    if a.large:
        rows.append(run("tile_1e7_k15", 10_000_000, 15, 64, a.reps, 2, dev))
    json.dump({"device": torch.cuda.get_device_name(0), "timing": "device events around the entry points, median of reps",
               "scenes": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
