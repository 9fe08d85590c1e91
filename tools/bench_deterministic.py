#!/usr/bin/env python
"""Time the deterministic training mode (csrc/loss_head_ordered.hip: the ordered loss-head backward and its list build) on
the GPU, on bench.py's default tile (``--n-tx`` 10^6 transcripts, ``--n-bd`` 10^4 boundaries, k = 15) staged as one batch of
a ``GraphedTrainer``:

* ``step_off_<dtype>``  the captured step with the flag off -- what every earlier commit replays; the tool runs unchanged on
                        a commit from before the mode (it then reports these records only): the before side;
* ``step_on_<dtype>``   the same with ``deterministic=True``;
* ``head_atomic`` / ``head_ordered``: the loss head alone (forward + backward through ``ops.loss_head``, the row
                        normalisation included, bf16) on the tile's shapes with uniformly drawn indices and one transcript row
                        that a tenth of the triplets name -- the skew a much-drawn cluster gives; ten calls captured into one
                        hipGraph so that a replay's fixed cost is shared.

Per record: ``--runs`` timings with device events, each around ``--steps`` replays; the median, minimum and maximum of the
per-step times.  One JSON line; ``--out`` also writes it to a file (profiles/deterministic_step_before_after.txt holds the
committed measurement).  No pass / fail bar."""
import argparse
import inspect
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
    ap.add_argument("--only", default="", help="comma separated subset of step_off,step_on,head")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_deterministic.py needs an MI355X: a CPU timing says nothing about it")
    from segger_amd import LitISTEncoder, ops
    from segger_amd.graph import csr_from_coo
    from segger_amd.synthetic import SyntheticSpec, make_graph
    from segger_amd.train_step_graph import GraphedTrainer
    dev = torch.device("cuda:0")
    has_mode = "deterministic" in inspect.signature(GraphedTrainer.__init__).parameters
    only = set(filter(None, args.only.split(",")))
    want = lambda name: not only or name in only

    spec = SyntheticSpec(n_tx=args.n_tx, n_bd=args.n_bd, k_tx=args.k, seed=0)
    batch_cpu, aux = make_graph(spec, return_aux=True)
    batch = batch_cpu.to(dev)

    def model(dtype):
        torch.manual_seed(0)
        m = LitISTEncoder(n_genes=spec.n_genes, in_channels=128)
        m.model._materialize_bd(spec.bd_dim, "cpu")
        m.model.compute_dtype = dtype
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

    res = {"tool": "bench_deterministic", "n_tx": args.n_tx, "n_bd": args.n_bd, "k": args.k, "has_mode": has_mode}
    for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        for name, kw in (("step_off", {}), ("step_on", dict(deterministic=True))):
            if not want(name) or (kw and not has_mode):
                continue
            m = model(dtype)
            tr = GraphedTrainer(m, m.configure_optimizers(capturable=True), **kw)
            for _ in range(3):
                tr.step(batch)
            res[f"{name}_{tag}"] = timed(lambda: tr.step(batch), 1)
            del tr, m
            torch.cuda.empty_cache()
    if want("head"):
        g = torch.Generator().manual_seed(0)
        n, nb, c = args.n_tx, args.n_bd, 64
        e = n // 2
        y, yb = torch.randn(n, c, generator=g).bfloat16().to(dev), torch.randn(nb, c, generator=g).bfloat16().to(dev)
        pos, neg = torch.randint(0, n, (n,), generator=g), torch.randint(0, n, (n,), generator=g)
        pos[::10] = 17                                                # one much-drawn row
        src, dst = torch.randperm(n, generator=g)[:e], torch.randint(0, nb, (e,), generator=g)
        dneg = (dst + torch.randint(1, nb, (e,), generator=g)) % nb
        groups = csr_from_coo(dst.to(dev), src.to(dev), nb, n, validate=False)
        of_tx = ops.anchor_index(src.to(dev), n)
        bd = tuple(t.to(dev) for t in (torch.randint(0, nb, (nb,), generator=g), torch.randint(0, nb, (nb,), generator=g),
                                       torch.rand(nb, generator=g), torch.rand(nb, generator=g), torch.full((nb,), 1.0 / nb)))
        a, b = torch.tensor([1.2, 1.0, 0.8], device=dev), torch.tensor([0.5, 0.2, 0.3], device=dev)
        hint = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev)
        tx = (torch.arange(n, device=dev), pos.to(dev), neg.to(dev), 0.3, 1e-6)
        sg = (src.to(dev), dst.to(dev), dneg.to(dev), 0.4, 1e-6, groups, True)
        res["head_rows"], res["head_hot_row_draws"] = n, n // 10

        def head(flag):
            yy, yyb = y.detach().requires_grad_(True), yb.detach().requires_grad_(True)
            zs = ops.l2_normalize_many({"tx": yy, "bd": yyb})
            kw = dict(deterministic=True) if flag else {}
            spec_ = ops.LossHeadSpec(tx, bd + (1e-8,), sg, tx_anchors_are_rows=True, sg_of_tx=of_tx, grad_out_hint=hint, **kw)
            torch.autograd.grad(ops.loss_head(zs["tx"], zs["bd"], a, b, spec_), (yy, yyb), hint)

        for name, flag in (("head_atomic", False), ("head_ordered", True)):
            if flag and not has_mode:
                continue
            head(flag)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(10):
                    head(flag)
            res[name] = timed(graph.replay, 10)
            res[name]["calls_per_replay"] = 10
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
