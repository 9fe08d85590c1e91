#!/usr/bin/env python
"""Time gradient accumulation in the captured training step (csrc/grad_accum.hip: segger_grad_accumulate and the windowed guard /
Adam) on the GPU, on bench.py's default tile (``--n-tx`` 10^6 transcripts, ``--n-bd`` 10^4 boundaries, k = 15, bf16 storage)
staged as one batch of a ``GraphedTrainer``:

* ``step_n1``      the captured step without accumulation -- what every earlier commit replays;
* ``micro_step``   a micro-step at ``accumulate_grad_batches=--n`` (every replay: backward, accumulate, predicated Adam);
* ``accumulate``   the accumulate launch by itself on the model's own gradients and accumulators, ten calls captured into
                   one hipGraph so that a replay's fixed cost is shared; beside it the bytes it moves (12 per element: the
                   gradient and the accumulator read, the accumulator written; 8 on a window's first micro-step) and what
                   they are of ``--peak-tbs`` TB/s.

Per record: ``--runs`` timings with device events, each around ``--steps`` replays, after a warm-up run; median, minimum and
maximum of the per-step times.  One JSON line; ``--out`` also writes it to a file
(profiles/grad_accumulation_bench_before_after.txt holds the committed measurement).  No pass / fail bar."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-tx", type=int, default=1_000_000)
    ap.add_argument("--n-bd", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--n", type=int, default=4, help="accumulate_grad_batches of the micro-step record")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_accumulation.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import LitISTEncoder, ops
    from segger_amd.synthetic import SyntheticSpec, make_graph
    from segger_amd.train_step_graph import GraphedTrainer
    dev = torch.device("cuda:0")
    spec = SyntheticSpec(n_tx=args.n_tx, n_bd=args.n_bd, k_tx=args.k, seed=0)
    batch_cpu, aux = make_graph(spec, return_aux=True)
    batch = batch_cpu.to(dev)

    def model():
        torch.manual_seed(0)
        m = LitISTEncoder(n_genes=spec.n_genes, in_channels=128)
        m.model._materialize_bd(spec.bd_dim, "cpu")
        m.model.compute_dtype = torch.bfloat16
        m = m.to(dev)
        m.set_similarities(aux["tx_similarity"].to(dev), aux["bd_similarity"].to(dev))
        m._max_epochs_override, m.current_epoch = 20, 10
        m.train()
        return m

    def timed(fn, per: int) -> dict:
        ms = []
        for r in range(args.runs + 1):                                # run 0 warms up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                ms.append(a.elapsed_time(b) / (args.steps * per))
        return {"median_us": round(1e3 * statistics.median(ms), 2), "min_us": round(1e3 * min(ms), 2),
                "max_us": round(1e3 * max(ms), 2), "runs": args.runs, "steps_per_run": args.steps}

    res = {"tool": "bench_grad_accumulation", "n_tx": args.n_tx, "n_bd": args.n_bd, "k": args.k, "dtype": "bf16", "n": args.n}
    for name, kw in (("step_n1", {}), ("micro_step", dict(accumulate_grad_batches=args.n))):
        m = model()
        tr = GraphedTrainer(m, m.configure_optimizers(capturable=True), **kw)
        for _ in range(args.n):
            tr.step(batch)
        res[name] = timed(lambda: tr.step(batch), 1)
        res[name]["captures"] = tr.n_captures
    # the accumulate launch alone: the micro-step trainer's own accumulators, gradients of their shapes
    window = tr.window
    params = [p for p in m.parameters() if p.grad is not None]
    raw = [torch.randn_like(p) for p in params]

    def call():
        for p, g in zip(params, raw):
            p.grad = g
        ops.grad_accumulate(params, window)
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(10):
            call()
    elements = sum(p.numel() for p in params)
    rec = timed(graph.replay, 10)
    moved = 12 * elements - 4 * elements / args.n                     # one launch in n is a window's first: no accumulator read
    rec.update(calls_per_replay=10, tensors=len(params), elements=elements, bytes_per_launch=int(moved),
               at_peak_us=round(moved / (args.peak_tbs * 1e12) * 1e6, 3),
               achieved_gbs=round(moved / (rec["median_us"] * 1e-6) / 1e9, 1))
    res["accumulate"] = rec
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
