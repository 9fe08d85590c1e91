"""The deterministic training mode on the GPU: the ordered loss-head backward (``ops.LossHeadSpec(deterministic=True)``,
segger_loss_head_ordered_fwd / _bwd) gives the same bytes launch after launch and captured against eager, agrees with its
float64 oracle (tests/loss_head_ordered_cases.py) and with the atomic route; a ``GraphedTrainer(deterministic=True)`` built
twice from one seed walks the same bytes step after step; the routes that add with float atomics are refused by name, and
with the flag off the head issues the library calls it always did.

The ordered route exposes no launch geometry (64 rows a workgroup, one workgroup a boundary are constants of the kernel),
so "another geometry" has nothing to vary here."""
import copy
import itertools

import numpy as np
import pytest
import torch

import loss_head_ordered_cases as lc

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# the tolerances tests/test_gpu_heads.py holds the atomic route to, per storage type: (losses: rtol, gradients: of the largest
# entry).  Measured maxima of the ordered route against the oracle on an MI355X are in the test's docstring below.
LOSS_TOL = {F32: 2e-6, BF16: 2e-2, F16: 3e-3}
GRAD_TOL = {F32: 5e-5, BF16: 3e-2, F16: 4e-3}
# transcript rows 0 .. 6 receive exactly 0, 1, 63, 64, 65, 200 and 400 contributions: both sides of the 64-term threshold
# between the serial and the 16-partial-sum form (and of the atomic route's chain capacity)
HOT = ((1, 1, 0), (2, 63, 0), (3, 64, 1), (4, 65, 0), (5, 200, 1), (6, 400, 0))
SMALL_HOT = ((1, 1, 1), (2, 63, 1), (3, 64, 0), (4, 65, 1))
# (n_tx, n_bd, C, dtype, kind, defer, prenorm): the whole product of boundary counts, widths, storage types, loss kinds and
# finish forms at 600 rows (every count above in every case), the un-normalised embeddings given in every other one; and two
# cases at 300 rows
CASES = [(600, n_bd, C, dtype, kind, defer, i % 2) for i, (n_bd, C, dtype, kind, defer) in enumerate(itertools.product(
    (1, 2, 7, 40), (32, 64, 128), (F32, BF16, F16), ("triplet", "bce"), (0, 1)))]
CASES += [(300, 40, 64, F32, "bce", 0, 1), (300, 7, 128, BF16, "triplet", 1, 0)]


def _problem(cuda, n_tx, n_bd, C, dtype, kind, prenorm):
    """The oracle's instance (margin 3: every loss_tx triplet is active, the counts above are exact), rounded to the storage
    type, on the device; the oracle's copy holds what the device reads."""
    from segger_amd import ops
    from segger_amd.graph import EdgeCSR
    p = lc.problem(n_tx=n_tx, n_bd=n_bd, n_sg=n_tx // 2, C=C, sg_kind=kind, seed=n_tx + n_bd + C, prenorm=bool(prenorm),
                   hot=HOT if n_tx >= 600 else SMALL_HOT, tx_margin=3.0)
    ok = (p["tx_pos"] >= 0)
    for row, count, _ in (HOT if n_tx >= 600 else SMALL_HOT):
        assert (p["tx_pos"][ok] == row).sum() + (p["tx_neg"][ok] == row).sum() == count
    assert not ((p["tx_pos"] == 0) | (p["tx_neg"] == 0)).any()
    if n_bd == 40:
        p["sg_neg"][p["sg_neg"] >= 0] = 11                          # every sampled negative on one boundary
        p["sg_pos"][p["sg_pos"] == 11] = 12
        p["sg_indptr"], p["sg_eid"] = lc.groups_by_positive(p["sg_pos"], n_bd)
    dev = lambda v, dt: torch.tensor(np.asarray(v), dtype=dt, device=cuda)
    y = dev(p["y_tx"] if prenorm else p["z_tx"], dtype)
    yb = dev(p["z_bd"], dtype)
    d = dict(y=y, yb=yb, prenorm=prenorm,
             tx=(torch.arange(n_tx, device=cuda), dev(p["tx_pos"], torch.int64), dev(p["tx_neg"], torch.int64), 3.0, 1e-6),
             bd=(dev(p["bd_pos"], torch.int64), dev(p["bd_neg"], torch.int64), dev(p["bd_dpos"], F32), dev(p["bd_dneg"], F32),
                 dev(p["bd_w"], F32), 1e-8),
             a=dev(p["a"], F32), b=dev(p["b"], F32), gvec=torch.tensor([1.0, 0.0, 0.5, 1.7], device=cuda), kind=kind, sg=None)
    if len(p["sg_src"]):
        indptr, eid = dev(p["sg_indptr"], torch.int64), dev(p["sg_eid"], torch.int32)
        groups = EdgeCSR(indptr, eid, eid, n_bd, n_tx)
        src = dev(p["sg_src"], torch.int64)
        d["sg"] = (src, dev(p["sg_pos"], torch.int64), dev(p["sg_neg"], torch.int64), 0.4, 1e-6, groups, True)
        d["of_tx"] = ops.anchor_index(src, n_tx)
    # what the device reads, for the oracle: the rounded rows; with prenorm the rows the normalisation kernel stored
    p["bd_dpos"], p["bd_dneg"], p["bd_w"] = (d["bd"][k].double().cpu().numpy() for k in (2, 3, 4))
    if prenorm:
        with torch.no_grad():
            zs = ops.l2_normalize_many({"tx": y, "bd": yb})
        p["y_tx"], p["z_tx"], p["z_bd"] = y.double().cpu().numpy(), zs["tx"].double().cpu().numpy(), zs["bd"].double().cpu().numpy()
        d["y_bd"] = yb.double().cpu().numpy()
    else:
        p["z_tx"], p["z_bd"] = y.double().cpu().numpy(), yb.double().cpu().numpy()
    return p, d


def _head(d, defer, deterministic=True):
    """One forward + backward -> (losses, grad of y_tx, grad of y_bd), fresh leaves."""
    from segger_amd import ops
    y, yb = d["y"].detach().clone().requires_grad_(True), d["yb"].detach().clone().requires_grad_(True)
    if d["prenorm"]:
        zs = ops.l2_normalize_many({"tx": y, "bd": yb})
        z, zb = zs["tx"], zs["bd"]
    else:
        z, zb = y, yb
    spec = ops.LossHeadSpec(d["tx"], d["bd"], d["sg"], sg_kind=d["kind"], tx_anchors_are_rows=True,
                            sg_of_tx=d.get("of_tx"), grad_out_hint=d["gvec"], defer_finish=bool(defer),
                            deterministic=deterministic)
    assert ops.loss_head_route(z, zb, spec) == ("one_launch_prenorm" if d["prenorm"] else "one_launch")
    res = ops.loss_head(z, zb, d["a"], d["b"], spec)
    gy, gyb = torch.autograd.grad(res, (y, yb), d["gvec"])
    return res.detach(), gy, gyb


def _bytes_equal(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.reshape(-1).contiguous().view(torch.uint8), y.reshape(-1).contiguous().view(torch.uint8))
               for x, y in zip(a, b))


@pytest.mark.parametrize("n_tx,n_bd,C,dtype,kind,defer,prenorm", CASES,
                         ids=lambda v: str(v).replace("torch.", "") if not isinstance(v, int) else None)
def test_ordered_head_repeats_its_bytes_and_matches_the_oracle(cuda, n_tx, n_bd, C, dtype, kind, defer, prenorm):
    """Five launches and one captured replay give identical bytes of the losses and of both gradients; the result is within
    the atomic route's tolerance of the float64 oracle and of the atomic route itself.

    Measured on an MI355X, largest over these cases as a fraction of the largest entry (against the oracle / against the
    atomic route): fp32 3.0e-6 / 1.6e-5, bf16 2.8e-3 / 1.6e-4, f16 3.1e-4 / 1.2e-4; the losses 2.9e-7.  The ordered route
    alone would support the historical 2e-5 at fp32; the distance to the atomic route (its own 400-term row in whatever
    order the atomics landed that day) sits too close under it, so both comparisons keep tests/test_gpu_heads.py's 5e-5."""
    p, d = _problem(cuda, n_tx, n_bd, C, dtype, kind, prenorm)
    runs = [tuple(t.clone() for t in _head(d, defer)) for _ in range(5)]
    assert all(torch.isfinite(t.float()).all() for t in runs[0])
    for r in runs[1:]:
        assert _bytes_equal(runs[0], r)
    # captured against eager (the step's form: everything the route needs comes out of the capture's pool)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _head(d, defer)
    graph.replay()
    torch.cuda.synchronize()
    assert _bytes_equal(runs[0], captured)
    # ---- correctness
    gout = d["gvec"].double().cpu().numpy()
    want_out = lc.losses(p)
    want_tx, want_bd = lc.gradients(p, gout)
    if prenorm:                                         # the boundary side's normalisation backward (its own launch)
        yb_ = d["y_bd"]
        nrm = np.linalg.norm(yb_, axis=1, keepdims=True)
        u = yb_ / nrm
        want_bd = (want_bd - u * (u * want_bd).sum(1, keepdims=True)) / nrm
    out, gy, gyb = (t.double().cpu().numpy() for t in runs[0])
    print(f"\nloss err {np.abs(out - want_out).max():.3e}")
    assert np.allclose(out, want_out, rtol=LOSS_TOL[dtype], atol=LOSS_TOL[dtype] * 1e-2)
    atomic = [t.double().cpu().numpy() for t in _head(d, defer, deterministic=False)]
    # a boundary that names ITSELF as positive or negative (certain with one boundary) has cos = 1 whatever the row: its own
    # loss_bd terms cancel analytically and what is left of them is rounding, relative to the terms -- 2 w |r| graw_1 <=
    # 2 w graw_1 each -- not to their sum; the largest entry is taken no smaller than that
    selfish = (p["bd_pos"] == np.arange(n_bd)) | (p["bd_neg"] == np.arange(n_bd))
    graw_1 = abs((gout[3] * p["b"][1] + gout[1]) * p["a"][1])
    floor = {"tx": 0.0, "bd": 2.0 * graw_1 * (p["bd_w"] * selfish).max()}
    for name, got, want, other in (("tx", gy, want_tx, atomic[1]), ("bd", gyb, want_bd, atomic[2])):
        scale = max(np.abs(want).max(), floor[name])
        err, apart = np.abs(got - want).max() / scale, np.abs(got - other).max() / scale
        print(f"grad_{name}: vs oracle {err:.3e}, vs atomic route {apart:.3e} (of the largest entry {scale:.3e})")
        assert scale > 0 and err <= GRAD_TOL[dtype] and apart <= GRAD_TOL[dtype], (name, err, apart)
    assert np.allclose(atomic[0], out, rtol=LOSS_TOL[dtype], atol=LOSS_TOL[dtype] * 1e-2)


def test_a_second_backward_gives_the_first_ones_bytes(cuda):
    from segger_amd import ops
    p, d = _problem(cuda, 300, 7, 64, F32, "triplet", 1)
    y, yb = d["y"].clone().requires_grad_(True), d["yb"].clone().requires_grad_(True)
    zs = ops.l2_normalize_many({"tx": y, "bd": yb})
    spec = ops.LossHeadSpec(d["tx"], d["bd"], d["sg"], sg_kind="triplet", tx_anchors_are_rows=True, deterministic=True)
    res = ops.loss_head(zs["tx"], zs["bd"], d["a"], d["b"], spec)
    first = torch.autograd.grad(res, (y, yb), d["gvec"], retain_graph=True)
    again = torch.autograd.grad(res, (y, yb), d["gvec"])
    assert _bytes_equal(first, again)


# ------------------------------------------------------------------------------------------------- refusals
def test_atomic_routes_are_refused_by_name(cuda, monkeypatch):
    from segger_amd import ops
    p, d = _problem(cuda, 300, 7, 64, F32, "triplet", 1)
    for prenorm, route in ((True, "anchor_rows"), (False, "kernel_by_kernel")):
        monkeypatch.setattr(ops, "ONE_LAUNCH_LOSS_HEAD", False)
        y, yb = d["y"].clone().requires_grad_(True), d["yb"].clone().requires_grad_(True)
        z = ops.l2_normalize_many({"tx": y, "bd": yb}) if prenorm else {"tx": y, "bd": yb}
        spec = ops.LossHeadSpec(d["tx"], d["bd"], d["sg"], tx_anchors_are_rows=True, deterministic=True)
        assert ops.loss_head_route(z["tx"], z["bd"], spec) == route
        with pytest.raises(NotImplementedError, match=route):
            ops.loss_head(z["tx"], z["bd"], d["a"], d["b"], spec)
        monkeypatch.setattr(ops, "ONE_LAUNCH_LOSS_HEAD", True)
    # a transcript that anchors two segmentation triplets: the one-launch head's atomic side launch
    sg = d["sg"][:6] + (False,)
    spec = ops.LossHeadSpec(d["tx"], d["bd"], sg, tx_anchors_are_rows=True, deterministic=True)
    with pytest.raises(NotImplementedError, match="segger_triplet_bwd"):
        ops.loss_head(d["y"].clone().requires_grad_(True), d["yb"], d["a"], d["b"], spec)
    spec = ops.LossHeadSpec(d["tx"], d["bd"], d["sg"][:6] + (lambda: False,), tx_anchors_are_rows=True, deterministic=True)
    y = d["y"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="segger_triplet_bwd"):        # a callable is asked in the backward
        ops.loss_head(y, d["yb"], d["a"], d["b"], spec)[3].backward()


def test_flag_off_makes_the_calls_it_always_made(cuda, monkeypatch):
    """The library calls of one forward + backward of the head, recorded: with the flag off the two entry points of the
    chained route and none of the ordered one (what the commit before made: segger_loss_head_fwd, segger_loss_head_bwd between
    the row normalisation's launches); with it on, the ordered pair in their place and nothing else changed."""
    from segger_amd import _lib
    p, d = _problem(cuda, 300, 7, 64, F32, "triplet", 1)
    real, calls = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("segger_") or name.endswith(("_bytes", "_rows", "_supported", "_error")):
                return fn
            def call(*a):
                calls.append(name)
                return fn(*a)
            return call

    monkeypatch.setattr(_lib, "load", lambda: Recorder())
    seen = {}
    for flag in (False, True):
        calls.clear()
        _head(d, 0, deterministic=flag)
        seen[flag] = list(calls)
    head = lambda names: [n for n in names if any(w in n for w in ("loss_head", "triplet", "metric", "loss_combine"))]
    rest = lambda names: [n for n in names if n not in head(names)]
    assert head(seen[False]) == ["segger_loss_head_fwd", "segger_loss_head_bwd"]
    assert head(seen[True]) == ["segger_loss_head_ordered_fwd", "segger_loss_head_ordered_bwd"]
    assert rest(seen[False]) == rest(seen[True]) and len(rest(seen[True])) >= 1           # (the row normalisation's launches)


def _captured_nodes(cuda, monkeypatch, tmp_path, dtype, **kw):
    """Nodes of the captured step of the step tests' model (tests/test_gpu_train_graph.py, 5000 transcripts, 170 boundaries)."""
    import re
    from segger_amd.synthetic import SyntheticSpec
    from segger_amd.train_step_graph import GraphedTrainStep, step_bucket
    from tests.test_gpu_train_graph import _model
    plain = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: plain(keep_graph=True))     # the hipGraph is kept for the dump
    m, bg = _model(SyntheticSpec(n_tx=5000, n_bd=170, k_tx=7, seed=31), cuda, dtype)
    step = GraphedTrainStep(m, m.configure_optimizers(capturable=True), step_bucket(bg, granularity=1.3), bg, **kw)
    step.step(bg, capture=True)
    torch.cuda.synchronize()
    assert step.graph is not None and step.graph_opt is None
    path = str(tmp_path / f"step_{len(kw)}.dot")
    step.graph.debug_dump(path)
    return len(dict(re.findall(r'"?(\w+)"?\s*\[[^\]]*label="([^"]*)"', open(path).read()))), step


@pytest.mark.parametrize("dtype,parent_nodes", [(F32, 87), (BF16, 50)], ids=["f32", "bf16"])
def test_flag_off_captures_the_step_it_always_did(cuda, monkeypatch, tmp_path, dtype, parent_nodes):
    """The captured step with the flag off has the node count of the commit before (recorded from it on an MI355X with this
    very function: 87 nodes at fp32, 50 at bf16) and keeps its deferred partial sums; with the flag on the head's two nodes
    become the ordered route's (keys, the sort's kernels, offsets, the backward) and the partial sums are launched where they
    are produced: more nodes, counted and printed, not pinned."""
    off, step = _captured_nodes(cuda, monkeypatch, tmp_path, dtype)
    assert off == parent_nodes and step.defer_sums and not step.deterministic
    on, step = _captured_nodes(cuda, monkeypatch, tmp_path, dtype, deterministic=True)
    print(f"\ncaptured nodes: flag off {off}, flag on {on}")
    assert on > off and step.deterministic and not step.defer_sums


def test_the_unfused_model_route_is_refused(cuda):
    from segger_amd.synthetic import SyntheticSpec
    from tests.test_gpu_train_graph import _model
    m, bg = _model(SyntheticSpec(n_tx=5000, n_bd=170, k_tx=7, seed=31), cuda, F32)
    m.deterministic = True
    losses = m.get_losses(bg)                                  # the fused eager path honours the flag
    assert torch.isfinite(losses[3])
    m.fused_loss_head = False
    with pytest.raises(NotImplementedError, match="unfused loss route"):
        m.get_losses(bg)


# ------------------------------------------------------------------------------------------------- the captured step
@pytest.fixture(scope="module")
def tiles(cuda):
    """The tile set of tests/test_gpu_train_graph.py's trainer test, and six batches that cross two shape buckets."""
    from segger_amd import tiles as T
    from segger_amd.synthetic import SyntheticSpec
    from tests.test_gpu_train_graph import _model
    made = {}

    def make(dtype):
        if dtype not in made:
            m, bg = _model(SyntheticSpec(n_tx=30000, n_bd=900, k_tx=6, seed=37), cuda, dtype)
            for nt in ("tx", "bd"):
                del bg[nt]["mask"]
            tiling = T.SquareTiling(torch.cat([bg["tx"].pos, bg["bd"].pos]).cpu(), 60.0)
            part = T.partition_by_tiling(bg, tiling, margin=3.0)
            part.build_csr()
            one = [[t] for t in range(len(part.node_sizes["tx"])) if part.node_sizes["bd"][t] > 1]
            one.sort(key=lambda ids: part.node_sizes["tx"][ids[0]])
            small, large = one[0], one[-1]
            assert part.node_sizes["tx"][large[0]] > 1.3 * part.node_sizes["tx"][small[0]]
            made[dtype] = (m, part, [small, large, small, one[len(one) // 2], large, small])
        return made[dtype]
    return make


def _trajectory(m, part, batches, **kw):
    from segger_amd.train_step_graph import GraphedTrainer
    m = copy.deepcopy(m)
    m.set_similarities(m.loss_tx.selector.similarity, m.loss_bd.selector.similarity)
    opt = m.configure_optimizers(capturable=True)
    trainer = GraphedTrainer(m, opt, granularity=1.1, deterministic=True, **kw)
    steps = []
    for ids in batches:
        out = trainer.step(part.batch(ids)).clone()
        torch.cuda.synchronize()
        state = [v.clone() for p_ in m.parameters() for _, v in sorted(opt.state[p_].items()) if isinstance(v, torch.Tensor)]
        steps.append([out] + [p_.detach().clone() for p_ in m.parameters()] + state
                     + ([trainer.guard.buf.clone()] if trainer.guard is not None else []))
    assert len(trainer.buckets) >= 2 and all(b.deterministic for b in trainer.buckets)
    assert int(m.model._step_dev) == 256 * len(batches)
    return steps


@pytest.mark.parametrize("dtype,guard", [(F32, False), (BF16, False), (F32, True)], ids=["f32", "bf16", "f32-guarded"])
def test_two_trainers_from_one_seed_walk_the_same_bytes(cuda, tiles, dtype, guard):
    """Six steps over two shape buckets, dropout on: parameters, Adam state and the four losses byte-identical after every
    step; with ``clip_grad_norm=1.0, loss_scale="dynamic"`` the guard's state too."""
    m, part, batches = tiles(dtype)
    kw = dict(clip_grad_norm=1.0, loss_scale="dynamic") if guard else {}
    first, second = _trajectory(m, part, batches, **kw), _trajectory(m, part, batches, **kw)
    for i, (a, b) in enumerate(zip(first, second)):
        assert len(a) == len(b) and torch.isfinite(a[0]).all()
        assert _bytes_equal(a, b), f"step {i}: {[k for k, (x, y) in enumerate(zip(a, b)) if not _bytes_equal([x], [y])][:5]}"
    assert not _bytes_equal(first[0][1:3], first[-1][1:3])          # it trained
