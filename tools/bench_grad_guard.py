#!/usr/bin/env python
"""Time the gradient guard of the captured training step (csrc/adam.hip: segger_grad_guard, segger_adam_step_guarded) on the
GPU, on bench.py's default tile (``--n-tx`` 10^6 transcripts, ``--n-bd`` 10^4 boundaries, k = 15, bf16 storage) staged as one
batch of a ``GraphedTrainer``:

* ``step_off``    the captured step without a guard -- what every earlier commit replays; the tool runs unchanged on a
                  commit from before the guard (it then reports this record only), which is how the before side is taken;
* ``step_on``     the same with ``clip_grad_norm=1.0, loss_scale="dynamic"``;
* ``guard_alone`` / ``adam_plain`` / ``guard_and_guarded_adam``: the optimizer launches by themselves on the model's own
                  parameters and gradients, ten calls captured into one hipGraph so that a replay's fixed cost is shared.

Per record: ``--runs`` timings with device events, each around ``--steps`` replays; the median, minimum and maximum of the
per-step times.  The steps train, as in a real epoch: the draws differ from step to step, the shapes do not.  One JSON line; ``--out`` also writes it to a file
(profiles/grad_guard_step_before_after.txt holds the committed measurement).  No pass / fail bar."""
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
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma separated subset of step_off,step_on,launches")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_guard.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import LitISTEncoder, ops
    from segger_amd.synthetic import SyntheticSpec, make_graph
    from segger_amd.train_step_graph import GraphedTrainer
    dev = torch.device("cuda:0")
    has_guard = hasattr(ops, "grad_guard")
    only = set(filter(None, args.only.split(",")))
    want = lambda name: not only or name in only

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

    res = {"tool": "bench_grad_guard", "n_tx": args.n_tx, "n_bd": args.n_bd, "k": args.k, "dtype": "bf16", "has_guard": has_guard}
    trainers = {}
    for name, kw in (("step_off", {}), ("step_on", dict(clip_grad_norm=1.0, loss_scale="dynamic"))):
        if not want(name) or (kw and not has_guard):
            continue
        m = model()
        tr = GraphedTrainer(m, m.configure_optimizers(capturable=True), **kw)
        for _ in range(3):
            tr.step(batch)
        res[name] = timed(lambda: tr.step(batch), 1)
        res[name]["captures"] = tr.n_captures
        if kw:
            g = tr.guard
            res[name].update(n_skipped=int(g.n_skipped), n_clipped=int(g.n_clipped), loss_scale=float(g.scale),
                             last_norm=float(g.norm))
        trainers[name] = (m, tr)
    if has_guard and want("launches") and trainers:
        m, tr = trainers.get("step_on") or trainers["step_off"]
        opt = tr.opt
        res["parameters"] = sum(p.numel() for p in m.parameters() if p.grad is not None)
        res["tensors"] = sum(1 for p in m.parameters() if p.grad is not None)
        state = ops.GuardState(dev, 1.0)
        hyper = torch.tensor(ops.adam_hyper(opt), dtype=torch.float64, device=dev)
        hyper[0] = 0.0                                                # rate 0: the timed updates leave the weights alone
        calls = {"guard_alone": lambda: ops.grad_guard(opt, state, max_norm=1.0, growth_interval=2000),
                 "adam_plain": lambda: ops.adam_step(opt, hyper_dev=hyper),
                 "guard_and_guarded_adam": lambda: (ops.grad_guard(opt, state, max_norm=1.0, growth_interval=2000),
                                                    ops.adam_step(opt, hyper_dev=hyper, guard=state))}
        for name, call in calls.items():
            call()                                                    # (workspace, lazy inits) before the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(10):
                    call()
            res[name] = timed(graph.replay, 10)
            res[name]["calls_per_replay"] = 10
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
