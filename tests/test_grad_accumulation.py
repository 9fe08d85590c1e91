"""Gradient accumulation in the captured training step (``GraphedTrainer(accumulate_grad_batches=N)``; csrc/grad_accum.hip:
segger_grad_accumulate, the windowed guard and Adam): a window of N micro-steps is ONE optimizer step on the sum of the
micro-gradients / N, decided on the device.  Batches are a few hundred transcripts and a few dozen boundaries: both edge
types and all three losses are live, every bucket sits on the ladder's floor or just above it.

Tolerance against eager torch (``close`` below): the one tests/test_gpu_train_graph.py's
test_graphed_step_gradients_equal_eager_step sets for the captured step against the eager one at N = 1, per tensor:
``|x - ref|.max() <= 2e-4 * |ref|.max() + 1e-7``."""
import copy
import types

import pytest
import torch

gpu = pytest.mark.gpu
F32 = torch.float32
INF = float("inf")


# ------------------------------------------------------------------------------------------------- helpers
def _spec(seed, n_tx=300, n_bd=24):
    from segger_amd.synthetic import SyntheticSpec
    return SyntheticSpec(n_tx=n_tx, n_bd=n_bd, k_tx=5, seed=seed)


@pytest.fixture(scope="module")
def world(cuda):
    """One model (the start of every run below, never stepped itself), three batches of one bucket, one of a larger bucket,
    and each batch's fixed draws -- made once, read by every test."""
    from segger_amd.synthetic import make_graph
    from tests.test_gpu_train_graph import _fixed_draws, _model
    base, a = _model(_spec(11), cuda, F32)
    batches = {"a": a, "b": make_graph(_spec(12)).to(cuda), "c": make_graph(_spec(13)).to(cuda),
               "big": make_graph(_spec(14, n_tx=520, n_bd=40)).to(cuda)}
    torch.manual_seed(3)
    draws = {k: _fixed_draws(base, bg) for k, bg in batches.items()}
    return types.SimpleNamespace(base=base, batches=batches, draws=draws)


def _twin(world, dropout: bool):
    m = copy.deepcopy(world.base)
    m.set_similarities(world.base.loss_tx.selector.similarity, world.base.loss_bd.selector.similarity)
    m.train()
    if not dropout:                                        # a batch's gradient must not depend on the dropout counter
        for mod in m.modules():
            if isinstance(getattr(mod, "dropout", None), float):
                mod.dropout = 0.0
    return m


def _trainer(world, n, dropout=False, **kw):
    from segger_amd.train_step_graph import GraphedTrainer
    m = _twin(world, dropout)
    opt = m.configure_optimizers(capturable=True)
    kw.setdefault("deterministic", True)
    if n is not None:
        kw["accumulate_grad_batches"] = n
    return m, opt, GraphedTrainer(m, opt, **kw)


def _set_draws(step, d):
    """Fixed draws of a batch in a bucket: handed over before the capture, rewritten IN PLACE afterwards (the graph reads
    these very tensors)."""
    from tests.test_gpu_train_graph import _pad_draws
    new = _pad_draws(step, d)
    if step.draws is None:
        step.draws = new
        return
    for dst, src in zip(step.draws["tx"] + step.draws["bd"] + (step.draws["dst_neg"],), new["tx"] + new["bd"] + (new["dst_neg"],)):
        dst.copy_(src)


def _step_fixed(world, tr, key):
    """``tr.step`` on batch ``key`` with that batch's fixed draws (the bucket is made first, so that its capture sees them)."""
    bg = world.batches[key]
    from segger_amd import capture as cap
    step = cap.pick(tr.buckets, bg, lambda: tr._capture(bg), tr.granularity, tr.max_buckets, "full")
    _set_draws(step, world.draws[key])
    out = tr.step(bg).clone()
    assert tr._last is step
    return out


def _state(m, opt, tr=None):
    """Everything a step may change, cloned: parameters, Adam's moments and counters, guard and window bytes, dropout counter."""
    torch.cuda.synchronize()
    out = {"p": [p.detach().clone() for p in m.parameters()], "m": [], "v": [], "t": [],
           "counter": int(m.model._step_dev)}
    for p in m.parameters():
        st = opt.state.get(p) or {}
        out["m"].append(st["exp_avg"].clone() if st else torch.zeros_like(p))
        out["v"].append(st["exp_avg_sq"].clone() if st else torch.zeros_like(p))
        out["t"].append(float(st["step"]) if st else 0.0)
    if tr is not None and tr.guard is not None:
        out["guard"] = tr.guard.buf.clone()
    return out


def _same(a, b, keys=("p", "m", "v", "t", "guard")):
    for k in keys:
        if k == "t":
            if a["t"] != b["t"]:
                return False
        elif k == "guard":
            if ("guard" in a) != ("guard" in b) or ("guard" in a and not torch.equal(a["guard"], b["guard"])):
                return False
        elif not all(torch.equal(x, y) for x, y in zip(a[k], b[k])):
            return False
    return True


def _eager_loss(m, bg, d):
    """The eager step's total loss with the draws given (tests/test_gpu_train_graph.py's _eager_grads, before its backward)."""
    from segger_amd import ops
    z = m(bg)
    n = bg["tx"].num_nodes
    l_tx = ops.triplet_edge_loss(z["tx"], None, torch.arange(n, device=z["tx"].device), *d["tx"], m.loss_tx.margin,
                                 eps=m.loss_tx.eps) * (n / bg["tx"]["mask"].sum().float())
    l_bd = ops.metric_loss(z["bd"], *d["bd"], d["bmask"].float() / d["bmask"].sum().float())
    l_sg = m._segmentation_loss(z, bg, d["dst_neg"])
    w = m._scheduled_weights(m._w_start, m._w_end)
    return float(w[0]) * l_tx + float(w[1]) * l_bd + float(w[2]) * l_sg


def _eager_window(world, keys, n):
    """Plain eager torch: sum of loss_i / n, backward, ONE torch.optim.Adam.step() -> (model, {name: gradient})."""
    m = _twin(world, dropout=False)
    opt = m.configure_optimizers()
    m.zero_grad(set_to_none=True)
    loss = sum(_eager_loss(m, world.batches[k], world.draws[k]) / n for k in keys)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    opt.step()
    torch.cuda.synchronize()
    return m, grads


def close(x, ref):
    err, bound = (x - ref).abs().max().item(), 2e-4 * ref.abs().max().item() + 1e-7
    return err <= bound, err, bound


def _against_eager(m, tr, eager, grads, what):
    worst_p = worst_g = 0.0
    for (k, p), (_, q) in zip(m.named_parameters(), eager.named_parameters()):
        ok, err, bound = close(p.detach(), q.detach())
        worst_p = max(worst_p, err / bound)
        assert ok, (what, "parameter", k, err, bound)
        if k in grads:
            ok, err, bound = close(tr.window.acc(p), grads[k])
            worst_g = max(worst_g, err / bound)
            assert ok, (what, "accumulated gradient", k, err, bound)
    print(f"\n{what}: worst error / bound: parameters {worst_p:.3e}, accumulated gradient {worst_g:.3e}")


# ------------------------------------------------------------------------------------------------- 1. exact identity
@gpu
@pytest.mark.parametrize("n", [2, 4])
def test_a_window_of_one_batch_repeated_is_the_single_step_byte_for_byte(cuda, world, n):
    """g/n summed n times is g exactly (n a power of two), so the window's update is the N = 1 step's: equal bytes in
    parameters, moments, counters and the guard's state.  After the first micro-step alone nothing has changed."""
    kw = dict(skip_nonfinite=True, loss_scale="dynamic")
    m1, o1, t1 = _trainer(world, None, **kw)
    _step_fixed(world, t1, "a")
    want = _state(m1, o1, t1)
    m, o, t = _trainer(world, n, **kw)
    start = _state(m, o, t)
    losses = []
    for i in range(n):
        losses.append(_step_fixed(world, t, "a"))
        if i == 0:
            first = _state(m, o, t)
            assert _same(first, start), "the first micro-step changed parameters, Adam state or the guard"
            assert int(t.window.pos) == 1 and int(t.window.close) == 0
    got = _state(m, o, t)
    assert all(torch.equal(x, losses[0]) for x in losses)
    assert got["t"] == want["t"] and max(got["t"]) == 1.0
    assert _same(got, want), "the window's update is not the single step's"
    assert int(t.window.pos) == 0 and int(t.window.close) == 1
    assert not _same(got, start, keys=("p",))


# ------------------------------------------------------------------------------------------------- 2. against eager torch
@gpu
def test_a_window_of_three_batches_against_eager_torch(cuda, world):
    keys = ("a", "b", "c")
    m, o, t = _trainer(world, 3)
    for k in keys:
        _step_fixed(world, t, k)
    assert len(t.buckets) == 1
    eager, grads = _eager_window(world, keys, 3)
    _against_eager(m, t, eager, grads, "N = 3, one bucket")
    assert all(float(o.state[p]["step"]) == 1.0 for p in m.parameters() if o.state.get(p))


# ------------------------------------------------------------------------------------------------- 3. a window across buckets
@gpu
def test_a_window_spans_two_buckets(cuda, world):
    m, o, t = _trainer(world, 2)
    replays = {}
    for key in ("a", "big"):                               # both buckets exist (and are counted) before the window opens
        bg = world.batches[key]
        step = t._capture(bg)
        t.buckets.append(step)
        replays[key] = 0
        def counted(empty=False, _real=step._replay, _key=key):
            replays[_key] += 1
            return _real(empty)
        step._replay = counted
    assert t.buckets[0].sizes["tx"] != t.buckets[1].sizes["tx"] and t.buckets[0].window is t.buckets[1].window is t.window
    ptrs = [a.data_ptr() for a in t.window.accumulators()]
    _step_fixed(world, t, "a")
    _step_fixed(world, t, "big")
    eager, grads = _eager_window(world, ("a", "big"), 2)
    _against_eager(m, t, eager, grads, "N = 2, two buckets")
    assert len(t.buckets) == 2 and all(b.graph is not None for b in t.buckets) and replays == {"a": 1, "big": 1}
    assert [a.data_ptr() for a in t.window.accumulators()] == ptrs
    assert all(p.grad is None or p.grad.data_ptr() == t.window.acc(p).data_ptr() for p in m.parameters())
    _step_fixed(world, t, "big")                            # a second window, the other way round: pure replays
    _step_fixed(world, t, "a")
    assert replays == {"a": 2, "big": 2} and t.n_captures == 2
    assert max(float(o.state[p]["step"]) for p in m.parameters() if o.state.get(p)) == 2.0


# ------------------------------------------------------------------------------------------------- 4. the guard
@gpu
def test_a_nonfinite_micro_batch_skips_the_whole_window_once(cuda, world):
    m, o, t = _trainer(world, 3, skip_nonfinite=True, loss_scale="dynamic")
    g = t.guard
    _step_fixed(world, t, "a")
    start = _state(m, o, t)
    t.window.accumulators()[0].view(-1)[0] = INF             # micro-batch 2 of 3 sums onto a non-finite value
    _step_fixed(world, t, "b")
    assert int(g.n_skipped) == 0 and float(g.scale) == 65536.0                    # nothing is decided before the close
    _step_fixed(world, t, "c")
    got = _state(m, o, t)
    assert _same(got, start, keys=("p", "m", "v", "t")) and max(got["t"]) == 0.0
    assert int(g.skipped) == 1 and int(g.n_skipped) == 1 and float(g.scale) == 32768.0 and torch.isnan(g.norm)
    for k in ("a", "b", "c"):                              # the next window, from finite batches, updates normally
        _step_fixed(world, t, k)
    after = _state(m, o, t)
    assert int(g.skipped) == 0 and int(g.n_skipped) == 1 and float(g.scale) == 32768.0 and int(g.growth_tracker) == 1
    assert max(after["t"]) == 1.0 and not _same(after, start, keys=("p",))
    assert all(torch.isfinite(p).all() for p in after["p"])


@gpu
def test_the_clip_is_decided_on_the_accumulated_norm(cuda, world):
    """The same batch twice, N = 2: the accumulated gradient is g, each term g / 2.  A bound of 0.75 |g| lies between the
    two -- clipped.  The converse with the first term turned into -0.4 g before the second is added: the sum is 0.1 g
    under a bound of 0.3 |g|, while each g / 2 alone is above it -- not clipped."""
    _, _, t0 = _trainer(world, None, clip_grad_norm=1e9)
    _step_fixed(world, t0, "a")
    norm = float(t0.guard.norm)
    assert norm > 0.0 and int(t0.guard.n_clipped) == 0
    _, _, t1 = _trainer(world, 2, clip_grad_norm=0.75 * norm)
    _step_fixed(world, t1, "a")
    assert int(t1.guard.n_clipped) == 0                    # (not decided yet)
    _step_fixed(world, t1, "a")
    print(f"\n|g| {norm!r}; accumulated {float(t1.guard.norm)!r}")
    assert int(t1.guard.n_clipped) == 1 and abs(float(t1.guard.norm) - norm) <= 1e-6 * norm and float(t1.guard.coef) < 1.0
    _, _, t2 = _trainer(world, 2, clip_grad_norm=0.3 * norm)
    _step_fixed(world, t2, "a")
    for a in t2.window.accumulators():
        a.mul_(-0.8)
    _step_fixed(world, t2, "a")
    print(f"accumulated after the turn {float(t2.guard.norm)!r} (0.1 |g| = {0.1 * norm!r})")
    # fp32: -0.8 (g/2) + g/2 loses ~ eps * 0.5 / 0.1 relative to the result, per element
    assert int(t2.guard.n_clipped) == 0 and abs(float(t2.guard.norm) - 0.1 * norm) <= 1e-5 * 0.1 * norm
    assert float(t2.guard.coef) == 1.0


# ------------------------------------------------------------------------------------------------- 5. counters
@gpu
def test_adam_counts_windows_and_the_dropout_counter_micro_steps(cuda, world):
    k, n = 2, 3
    order = ["a", "b", "c", "a", "c", "b"]
    m, o, t = _trainer(world, n, dropout=True)
    for key in order:
        t.step(world.batches[key])
    m1, o1, t1 = _trainer(world, None, dropout=True)
    for key in order[:k]:
        t1.step(world.batches[key])
    adam_after_k = _state(m1, o1)["t"]
    for key in order[k:]:
        t1.step(world.batches[key])
    counter_after_kn = int(m1.model._step_dev)
    got = _state(m, o)
    assert got["t"] == adam_after_k and max(got["t"]) == float(k)
    assert got["counter"] == counter_after_kn == 256 * k * n


# ------------------------------------------------------------------------------------------------- 6. flush
@gpu
def test_flush_applies_the_open_window_and_the_next_one_starts_clean(cuda, world):
    m, o, t = _trainer(world, 4, skip_nonfinite=True)
    t.flush()                                              # nothing captured, nothing open
    _step_fixed(world, t, "a")
    _step_fixed(world, t, "b")
    assert int(t.window.pos) == 2 and not t.window_closed
    t.flush()
    assert int(t.window.pos) == 0 and t.window_closed
    eager, grads = _eager_window(world, ("a", "b"), 4)      # (g1 + g2) / 4
    _against_eager(m, t, eager, grads, "N = 4, flushed after two")
    once = _state(m, o, t)
    assert max(once["t"]) == 1.0 and int(t.guard.n_skipped) == 0
    t.flush()
    assert _same(_state(m, o, t), once), "a second flush changed something"
    for a in t.window.accumulators():
        a.fill_(1e30)                                      # the next window must OVERWRITE, not add
    _step_fixed(world, t, "c")
    assert int(t.window.pos) == 1
    assert all(float(a.abs().max()) < 1e3 for a in t.window.accumulators())
    assert _same(_state(m, o, t), once)


# ------------------------------------------------------------------------------------------------- 7. determinism
@gpu
def test_two_runs_from_one_seed_give_the_same_bytes_after_every_micro_step(cuda, world):
    order = ["a", "big", "b", "big", "big", "c"]
    runs = [_trainer(world, 3, dropout=True, skip_nonfinite=True, loss_scale="dynamic", clip_grad_norm=1.0) for _ in range(2)]
    for i, key in enumerate(order):
        outs, states = [], []
        for m, o, t in runs:
            outs.append(t.step(world.batches[key]).clone())
            states.append((_state(m, o, t), t.window.buf.clone(), [a.clone() for a in t.window.accumulators()]))
        assert torch.equal(outs[0], outs[1]), i
        assert _same(states[0][0], states[1][0]) and states[0][0]["counter"] == states[1][0]["counter"], i
        assert torch.equal(states[0][1], states[1][1]) and all(torch.equal(x, y) for x, y in zip(states[0][2], states[1][2])), i
    m, o, t = runs[0]
    assert len(t.buckets) == 2 and max(_state(m, o)["t"]) == 2.0 and int(t.guard.n_skipped) == 0


# ------------------------------------------------------------------------------------------------- 8. refusals and default
def _cpu_pair():
    from segger_amd import LitISTEncoder
    m = LitISTEncoder(n_genes=16, in_channels=8, hidden_channels=8, out_channels=8)
    params = [p for p in m.parameters() if not isinstance(p, torch.nn.parameter.UninitializedParameter)]
    return m, params


def test_bad_window_lengths_and_unsupported_combinations_are_refused(monkeypatch):
    from segger_amd import LitISTEncoder
    from segger_amd.train_step_graph import GraphedTrainer
    m, params = _cpu_pair()
    adam = torch.optim.Adam(params, lr=1e-3, capturable=True)
    for bad in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="accumulate_grad_batches must be an int >= 1"):
            GraphedTrainer(m, adam, accumulate_grad_batches=bad)
    with pytest.raises(ValueError, match="accumulate_grad_batches must be an int >= 1"):
        m.enable_graphed_training(accumulate_grad_batches=0)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        GraphedTrainer(m, adam, accumulate_grad_batches=2, grad_sync=lambda: None)
    for opt in (torch.optim.AdamW(params, lr=1e-3, capturable=True), torch.optim.SGD(params, lr=1e-3),
                torch.optim.Adam(params, lr=1e-3, capturable=True, weight_decay=0.1)):
        with pytest.raises(NotImplementedError, match="does not cover this optimizer"):
            GraphedTrainer(m, opt, accumulate_grad_batches=2)
    # N = 1 with any of them is what it always was: accepted, nothing allocated
    for kw in (dict(grad_sync=lambda: None), {}):
        t = GraphedTrainer(m, adam, accumulate_grad_batches=1, **kw)
        assert t.window is None and t.accumulate_grad_batches == 1 and t.window_closed
    assert GraphedTrainer(m, adam).accumulate_grad_batches == 1
    t = GraphedTrainer(m, adam, accumulate_grad_batches=3)
    assert t.accumulate_grad_batches == 3 and t.window is None            # (made with the first bucket, on the device)
    t.flush()                                                             # nothing open: nothing happens
    # the public spellings
    m.enable_graphed_training(accumulate_grad_batches=3)
    assert m._graphed_kw["accumulate_grad_batches"] == 3
    m.enable_graphed_training()
    assert "accumulate_grad_batches" not in m._graphed_kw
    m.fast(accumulate_grad_batches=2)
    assert m._graphed_kw["accumulate_grad_batches"] == 2
    monkeypatch.setenv("SEGGER_AMD_ACCUMULATE", "4")
    monkeypatch.setenv("SEGGER_AMD_GRAPHED", "1")
    assert LitISTEncoder(n_genes=16, in_channels=8)._graphed_kw["accumulate_grad_batches"] == 4
    monkeypatch.setenv("SEGGER_AMD_ACCUMULATE", "1")
    assert "accumulate_grad_batches" not in LitISTEncoder(n_genes=16, in_channels=8)._graphed_kw
    for bad in ("0", "1.5", "many"):
        monkeypatch.setenv("SEGGER_AMD_ACCUMULATE", bad)
        with pytest.raises(ValueError, match="must be an int >= 1"):
            LitISTEncoder(n_genes=16, in_channels=8)


@gpu
def test_without_accumulation_the_captured_step_is_the_one_it_always_was(cuda, world, monkeypatch, tmp_path):
    """N = 1: no accumulator, and the node count tests/test_gpu_loss_head_ordered.py pins for the commit before (87 at fp32,
    its model and bucket); N = 2 adds its launches (printed, not pinned)."""
    from tests.test_gpu_loss_head_ordered import _captured_nodes
    nodes, step = _captured_nodes(cuda, monkeypatch, tmp_path, F32, accumulate_grad_batches=1)
    assert nodes == 87 and step.window is None and step.graph_flush is None
    more, step = _captured_nodes(cuda, monkeypatch, tmp_path, F32, accumulate_grad_batches=2, deterministic=False)
    print(f"\ncaptured nodes: N = 1: {nodes}, N = 2: {more}")
    assert more > nodes and step.window is not None and int(step.window.pos) == 1
    _, _, t = _trainer(world, 1)
    t.step(world.batches["a"])
    assert t.window is None and t.buckets[0].window is None


@gpu
def test_under_lightning_the_window_closes_at_the_epoch_end(cuda, world):
    """``enable_graphed_training(accumulate_grad_batches=2)``: global_step counts closed windows, ``on_train_epoch_end``
    flushes an open one; a Trainer asking for accumulation itself while the module was not told gets a warning."""
    class Progress:
        ready = completed = 0

    class Wrapper:
        def __init__(self, optimizer, prog):
            self.optimizer = optimizer
            self._on_before_step = lambda: setattr(prog, "ready", prog.ready + 1)
            self._on_after_step = lambda: setattr(prog, "completed", prog.completed + 1)
    m = _twin(world, dropout=True)
    m.enable_graphed_training(accumulate_grad_batches=2)
    opt = m.configure_optimizers()
    prog = Progress()
    m.trainer = types.SimpleNamespace(optimizers=[Wrapper(opt, prog)], max_epochs=20, datamodule=None, accumulate_grad_batches=1)
    for i, key in enumerate(("a", "b", "c")):
        assert torch.isfinite(m.training_step(world.batches[key], i))
    assert (prog.ready, prog.completed) == (1, 1)
    m.on_train_epoch_end()
    assert (prog.ready, prog.completed) == (2, 2) and m._graphed_trainer.window_closed
    assert max(float(opt.state[p]["step"]) for p in m.parameters() if opt.state.get(p)) == 2.0
    m.on_train_epoch_end()
    assert (prog.ready, prog.completed) == (2, 2)
    quiet = _twin(world, dropout=True)
    quiet.enable_graphed_training()
    qopt = quiet.configure_optimizers()
    quiet.trainer = types.SimpleNamespace(optimizers=[qopt], max_epochs=20, datamodule=None, accumulate_grad_batches=4)
    with pytest.warns(UserWarning, match=r"enable_graphed_training\(accumulate_grad_batches=4\)"):
        quiet.training_step(world.batches["a"], 0)


# ------------------------------------------------------------------------------------------------- the C ABI (no device)
def test_the_abi_entries_exist_and_reject_bad_arguments_on_the_host():
    """Nothing is launched: every pointer is a fake aligned address that a rejected call never dereferences."""
    import ctypes as C
    from segger_amd import _lib, ops
    lib = _lib.load()
    EINVAL, FAKE = -1, 0x1000
    err = lambda: lib.segger_last_error() if hasattr(lib, "segger_last_error") else b""
    for name in ("segger_grad_accumulate", "segger_grad_guard_windowed", "segger_adam_step_windowed", "segger_accum_window_flush"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.segger_abi_version() == 32 == _lib.ABI_VERSION              # purely additive
    W = _lib.AccumWindow
    assert C.sizeof(W) == 16 and [(n, getattr(W, n).offset) for n, _ in W._fields_] == [
        ("pos", 0), ("close", 4), ("arrived", 8), ("reserved_", 12)]
    for name in ("GradWindow", "grad_accumulate", "window_flush", "accumulate_batches"):
        assert hasattr(ops, name)

    def table(**bad):
        arr = (_lib.AdamTensor * 2)()
        for a in arr:
            a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.step, a.numel = FAKE, 2 * FAKE, FAKE, FAKE, FAKE, 5000
        for k, v in bad.items():
            setattr(arr[0], k, v)
        return arr
    acc = lambda tensors=None, n=2, n_window=4, window=FAKE: lib.segger_grad_accumulate(tensors or table(), n, n_window, window, None)
    assert acc(n_window=0) == EINVAL and acc(n_window=-3) == EINVAL
    assert acc(window=None) == EINVAL and acc(window=FAKE + 2) == EINVAL
    assert acc(n=-1) == EINVAL
    assert acc(table(numel=-1)) == EINVAL and acc(table(grad=None)) == EINVAL and acc(table(param=None)) == EINVAL
    assert acc(table(grad=FAKE)) == EINVAL                                  # the accumulator must not be the gradient
    assert acc(table(grad=2 * FAKE + 2)) == EINVAL                          # misaligned
    cfg = _lib.GuardCfg(1.0, 2.0, 0.5, 2000, 0)
    assert lib.segger_grad_guard_windowed(table(), 2, C.byref(cfg), FAKE, FAKE, 1 << 20, None, None) == EINVAL
    advanced = _lib.GuardCfg(1.0, 2.0, 0.5, 2000, _lib.ADAM_STEPS_ADVANCED)
    assert lib.segger_grad_guard_windowed(table(), 2, C.byref(advanced), FAKE, FAKE, 1 << 20, FAKE, None) == EINVAL
    assert lib.segger_grad_guard_windowed(None, 0, C.byref(cfg), FAKE, FAKE, 1 << 20, FAKE, None) == 0      # empty: nothing to do
    step = lambda hyper=FAKE, flags=0, state=None, window=FAKE: lib.segger_adam_step_windowed(table(), 2, hyper, flags, None, 0, state, window, None)
    assert step(hyper=None) == EINVAL and step(window=None) == EINVAL and step(state=FAKE + 4) == EINVAL
    assert step(flags=_lib.ADAM_STEPS_ADVANCED) == EINVAL
    assert lib.segger_accum_window_flush(None, 0, None) == EINVAL and lib.segger_accum_window_flush(FAKE, 2, None) == EINVAL
