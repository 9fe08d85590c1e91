"""Times the phenograph clustering on one MI355X and writes profiles/phenograph_cells_per_s.json (reported, not gated).

Synthetic X [N, 128] from 8 cell types, k = 10, resolution 2.  Per stage and in total: the median of 5 runs after a
warm-up, host clock around a device synchronise.  The kNN is timed against the formulation a user has today -- chunked
``X_chunk @ X.T`` + norms + ``torch.topk`` in fp32 on the same device -- the two paths alternating run by run, with the
peak memory above the inputs of each.  Louvain has no device baseline: its time, levels, rounds and Q stand alone.  Every
size runs in a child process of its own under a time limit, and the tool stops at the first failure.

    python tools/bench_phenograph.py [--sizes 100000 1000000] [--limit 900]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_MFMA = 157.3e12


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def peak_above(fn, torch):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def baseline_knn(X, k, torch, chunk=4096):
    sq = (X * X).sum(dim=1)
    idx = torch.empty(X.shape[0], k, dtype=torch.int64, device=X.device)
    for s in range(0, X.shape[0], chunk):
        score = sq[s:s + chunk, None] + sq[None, :] - 2.0 * (X[s:s + chunk] @ X.T)
        idx[s:s + chunk] = torch.topk(score, k, dim=1, largest=False).indices
    return idx


def run_size(n, runs):
    import torch
    from segger_amd import phenograph as pg
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    centres = 12.0 / 128 ** 0.5 * torch.randn(8, 128, generator=gen)
    X = (centres[torch.randint(0, 8, (n,), generator=gen)] + torch.randn(n, 128, generator=gen)).to(dev)
    X = X - X.mean(dim=0, keepdim=True)
    pg.knn_bruteforce(X[:4096].contiguous(), 10)                       # warm-up of both paths
    baseline_knn(X[:8192].contiguous(), 10, torch)
    mem_new, (idx, _) = peak_above(lambda: pg.knn_bruteforce(X, 10), torch)
    mem_old, idx_old = peak_above(lambda: baseline_knn(X, 10, torch), torch)
    agree = float((idx.long().sort(dim=1).values == idx_old.sort(dim=1).values).all(dim=1).float().mean())
    t_new, t_old = [], []
    for _ in range(runs):                                              # alternating
        t_new.append(timed(lambda: pg.knn_bruteforce(X, 10), torch)[0])
        t_old.append(timed(lambda: baseline_knn(X, 10, torch), torch)[0])
    t_jac, t_lou, t_all = [], [], []
    graph = pg.jaccard_graph(idx)
    labels, q, stats = pg.louvain(*graph, resolution=2.0, return_stats=True)
    for _ in range(runs):
        t_jac.append(timed(lambda: pg.jaccard_graph(idx), torch)[0])
        t_lou.append(timed(lambda: pg.louvain(*graph, resolution=2.0), torch)[0])
        t_all.append(timed(lambda: pg.phenograph(X, 10, 2.0), torch)[0])
    knn_s = statistics.median(t_new)
    flop = 2.0 * n * n * 128
    return {"n": n, "d": 128, "k": 10, "resolution": 2.0, "runs": runs,
            "knn_s": knn_s, "knn_baseline_s": statistics.median(t_old), "knn_all_s": t_new, "knn_baseline_all_s": t_old,
            "knn_peak_bytes": mem_new, "knn_baseline_peak_bytes": mem_old, "knn_rows_with_the_baseline_s_set": agree,
            "knn_tflops": flop / knn_s / 1e12, "knn_fraction_of_fp32_mfma_peak": flop / knn_s / PEAK_FP32_MFMA,
            "jaccard_s": statistics.median(t_jac), "edges": int(graph[1].numel()),
            "louvain_s": statistics.median(t_lou), "louvain_levels": stats["levels"], "louvain_rounds": stats["rounds"],
            "louvain_q": q, "clusters": int(labels.max()) + 1, "total_s": statistics.median(t_all),
            "cells_per_s": n / statistics.median(t_all)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds per size")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phenograph_cells_per_s.json"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(run_size(args.child, args.runs)))
        return
    results = []
    for n in args.sizes:                                               # a fresh process per size, each under its own limit
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--runs", str(args.runs)],
                              capture_output=True, text=True, timeout=args.limit)
        if proc.returncode != 0:
            sys.exit(f"N = {n} failed with status {proc.returncode}; stopping here\n{proc.stderr[-2000:]}")
        line = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        results.append(json.loads(line[7:]))
        print(line[7:], flush=True)
    with open(args.out, "w") as f:
        json.dump({"device": "MI355X", "fp32_mfma_peak_flops": PEAK_FP32_MFMA, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
