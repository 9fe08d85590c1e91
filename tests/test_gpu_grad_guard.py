"""The gradient guard on the device (segger_grad_guard, segger_adam_step_guarded; ops.grad_guard / adam_step(guard=) and the
captured step's ``clip_grad_norm`` / ``loss_scale`` / ``skip_nonfinite``) against the float64 oracle of
tests/grad_guard_cases.py and torch's own fused Adam.  A non-finite gradient is ordinary data to these kernels."""
import copy
import types

import numpy as np
import pytest
import torch

from tests import grad_guard_cases as G

pytestmark = pytest.mark.gpu

SHAPES = [(384, 128), (128,), (1, 2, 64), (7,), (3, 5), (0,), (64, 130), (1,), (2049,), (4096,)]
MANY = [(3,), (2048,), (0,), (5, 7), (2050,)] * 13                     # 65 tensors: a second batch of the launch table


def _read(state):
    """The device struct, parsed on the host."""
    from segger_amd import _lib
    torch.cuda.synchronize()
    return _lib.GuardState.from_buffer_copy(bytes(state.buf.cpu().numpy().tobytes()))


def _set(state, st):
    state.scale.fill_(float(st["scale"]))
    state.growth_tracker.fill_(st["growth_tracker"])
    state.n_skipped.fill_(st["n_skipped"])
    state.n_clipped.fill_(st["n_clipped"])


def _optimizer(shapes, dev, gen, lr=1e-3):
    ps = [torch.randn(s, device=dev, generator=gen).requires_grad_(True) for s in shapes]
    return ps, torch.optim.Adam(ps, lr=lr, fused=True, capturable=True)


def _ulp_close(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) <= float(np.spacing(np.abs(b)))


def _check_against_oracle(got, want, n_elements):
    assert got.skip == want["skip"] and got.growth_tracker == want["growth_tracker"]
    assert (got.n_skipped, got.n_clipped) == (want["n_skipped"], want["n_clipped"])
    if want["skip"]:
        assert np.isnan(got.norm) and got.coef == 0.0
    else:
        bound = (n_elements + 2) * 2.0 ** -53                          # plain double summation of n terms, sqrt, one division
        print(f"norm {got.norm!r} oracle {want['norm']!r} rel {abs(got.norm - want['norm']) / max(want['norm'], 1e-300):.3e} bound {bound:.3e}")
        assert abs(got.norm - want["norm"]) <= bound * want["norm"]
        assert _ulp_close(got.coef, want["coef"]), (got.coef, want["coef"])
    assert _ulp_close(got.scale, want["scale"]), (got.scale, want["scale"])


@pytest.mark.parametrize("shapes", [SHAPES, MANY], ids=["ten_tensors", "sixty_five_tensors"])
@pytest.mark.parametrize("cfg,before", [
    (G.config(max_norm=1.0, growth_interval=3), G.fresh_state(1024.0, growth_tracker=2, n_clipped=5)),
    (G.config(max_norm=0.0), G.fresh_state(1.0)),
    (G.config(max_norm=1e9, growth_interval=2000), G.fresh_state(65536.0, growth_tracker=7)),
], ids=["clip_dynamic_grows", "off_static", "loose_dynamic"])
def test_guard_matches_the_oracle_and_repeats_its_bytes(cuda, shapes, cfg, before):
    from segger_amd import ops
    gen = torch.Generator(device=cuda).manual_seed(7)
    ps, opt = _optimizer(shapes, cuda, gen)
    for p in ps:
        p.grad = torch.randn(p.shape, device=cuda, generator=gen) * float(before["scale"]) * 0.01
    ops.adam_init_state(opt)
    steps = [opt.state[p]["step"] for p in ps]
    state = ops.GuardState(cuda)
    n = sum(p.numel() for p in ps)
    kw = {k: cfg[k] for k in ("max_norm", "growth", "backoff", "growth_interval")}
    runs = []
    for _ in range(2):
        _set(state, before)
        ops.grad_guard(opt, state, **kw)
        runs.append(state.buf.cpu().clone())
    assert torch.equal(runs[0], runs[1])                               # the same gradients: the same bytes
    want = G.guard_step([p.grad.cpu().numpy() for p in ps], before, cfg)
    _check_against_oracle(_read(state), want, n)
    assert all(float(s) == 0.0 for s in steps)                         # a clean step: the guard leaves the counters alone
    # the hand-worked special values, on the device: one inf / one NaN in the scalar tail of an odd tensor / all zero
    for value, where in ((float("inf"), 0), (float("nan"), 3), (float("nan"), len(ps) - 1)):
        keep = ps[where].grad.clone()
        ps[where].grad.view(-1)[-1] = value
        _set(state, before)
        ops.grad_guard(opt, state, **kw)
        _check_against_oracle(_read(state), G.guard_step([p.grad.cpu().numpy() for p in ps], before, cfg), n)
        assert _read(state).skip == 1
        ps[where].grad.copy_(keep)
    for p in ps:
        p.grad.zero_()
    _set(state, before)
    ops.grad_guard(opt, state, **kw)
    got = _read(state)
    _check_against_oracle(got, G.guard_step([p.grad.cpu().numpy() for p in ps], before, cfg), n)
    assert got.norm == 0.0 and got.coef == np.float32(1.0 / float(before["scale"]))


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_guard_gives_the_hand_worked_numbers(cuda, case):
    from segger_amd import ops
    _, grads, before, cfg, want = case
    ps = [torch.zeros(np.asarray(g).shape, device=cuda, requires_grad=True) for g in grads]
    opt = torch.optim.Adam(ps, lr=1e-3, fused=True, capturable=True)
    for p, g in zip(ps, grads):
        p.grad = torch.tensor(np.asarray(g, dtype=np.float32), device=cuda)
    ops.adam_init_state(opt)
    state = ops.GuardState(cuda)
    _set(state, before)
    ops.grad_guard(opt, state, **cfg)
    _check_against_oracle(_read(state), want, sum(p.numel() for p in ps))


def test_guarded_adam_matches_torch_adam_on_prescaled_gradients(cuda):
    """Six steps under a dynamic scale that grows every second step, clipped at 1: ours = guard + guarded Adam on the scaled
    gradients; torch's fused capturable Adam is fed the oracle's ``g * coef``.  test_adam_kernel_matches_torch_adam's
    tolerance: its allowance covers the one extra rounding of ``g * coef``."""
    from segger_amd import ops
    gen = torch.Generator(device=cuda).manual_seed(5)
    ps_a, oa = _optimizer(SHAPES, cuda, gen)
    ps_b = [p.detach().clone().requires_grad_(True) for p in ps_a]
    ob = torch.optim.Adam(ps_b, lr=1e-3, fused=True, capturable=True)
    cfg = G.config(max_norm=1.0, growth_interval=2)
    st = G.fresh_state(1024.0)
    state = ops.GuardState(cuda, 1024.0)
    for step in range(6):
        grads = [torch.randn(s, device=cuda, generator=gen) * (10.0 ** (step % 3 - 1)) * float(st["scale"]) * 1e-3 for s in SHAPES]
        want = G.guard_step([g.cpu().numpy() for g in grads], st, cfg)
        for p, q, gr in zip(ps_a, ps_b, grads):
            p.grad, q.grad = gr.clone(), gr * float(want["coef"])
        ops.adam_init_state(oa)
        ops.grad_guard(oa, state, max_norm=1.0, growth_interval=2)
        assert ops.adam_step(oa, guard=state)
        ob.step()
        _check_against_oracle(_read(state), want, sum(p.numel() for p in ps_a))
        st = G.next_state(want)
        for p, q in zip(ps_a, ps_b):
            sa, sb = oa.state[p], ob.state[q]
            assert float(sa["step"]) == float(sb["step"]) == step + 1
            for x, y in ((p, q), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
                scale = float(y.abs().max()) if y.numel() else 0.0
                assert torch.allclose(x, y, rtol=2e-6, atol=5e-7 * scale + 1e-12), (step, tuple(p.shape))
    assert float(state.scale) == 8192.0 and int(state.n_skipped) == 0


@pytest.mark.parametrize("advanced", [False, True], ids=["adam_advances", "counters_advanced_at_the_head"])
def test_a_skipped_step_changes_nothing_but_the_counter_and_the_scale(cuda, advanced):
    from segger_amd import ops
    gen = torch.Generator(device=cuda).manual_seed(9)
    ps_a, oa = _optimizer(SHAPES, cuda, gen)
    ps_b = [p.detach().clone().requires_grad_(True) for p in ps_a]
    ob = torch.optim.Adam(ps_b, lr=1e-3, fused=True, capturable=True)
    state = ops.GuardState(cuda, 1024.0)
    counter = torch.zeros(1, dtype=torch.int64, device=cuda)
    kw = dict(max_norm=0.0, growth_interval=1000)

    def ours(grads):
        for p, gr in zip(ps_a, grads):
            p.grad = gr.clone()
        ops.adam_init_state(oa)
        if advanced:                                                   # what the draws launch does at the head of a captured step
            torch._foreach_add_([oa.state[p]["step"] for p in ps_a], 1.0)
        ops.grad_guard(oa, state, steps_advanced=advanced, **kw)
        assert ops.adam_step(oa, steps_advanced=advanced, counter=counter, counter_inc=256, guard=state)

    def theirs(grads, coef):
        for q, gr in zip(ps_b, grads):
            q.grad = gr * coef
        ob.step()

    clean = lambda scale: [torch.randn(s, device=cuda, generator=gen) * scale for s in SHAPES]
    g0 = clean(1024.0)
    ours(g0); theirs(g0, 1.0 / 1024.0)
    keep = [(p.detach().clone(), oa.state[p]["exp_avg"].clone(), oa.state[p]["exp_avg_sq"].clone(), float(oa.state[p]["step"]))
            for p in ps_a]
    g1 = clean(1024.0)
    g1[6].view(-1)[1234] = float("inf")
    ours(g1)                                                           # skipped
    got = _read(state)
    assert (got.skip, got.n_skipped, got.scale, got.growth_tracker) == (1, 1, 512.0, 0) and int(counter) == 512
    for p, (w, m, v, s) in zip(ps_a, keep):
        assert torch.equal(p.detach(), w) and torch.equal(oa.state[p]["exp_avg"], m) and torch.equal(oa.state[p]["exp_avg_sq"], v)
        assert float(oa.state[p]["step"]) == s == 1.0
    g2 = clean(512.0)                                                  # the next clean step is torch's next step
    ours(g2); theirs(g2, 1.0 / 512.0)
    assert _read(state).skip == 0 and int(counter) == 768
    for p, q in zip(ps_a, ps_b):
        sa, sb = oa.state[p], ob.state[q]
        assert float(sa["step"]) == float(sb["step"]) == 2.0
        for x, y in ((p, q), (sa["exp_avg"], sb["exp_avg"]), (sa["exp_avg_sq"], sb["exp_avg_sq"])):
            scale = float(y.abs().max()) if y.numel() else 0.0
            assert torch.allclose(x, y, rtol=2e-6, atol=5e-7 * scale + 1e-12), tuple(p.shape)


def test_a_guard_on_an_uncovered_optimizer_is_an_error(cuda):
    from segger_amd import ops
    from segger_amd.train_step_graph import make_guard, guard_config
    p = torch.zeros(8, device=cuda, requires_grad=True)
    p.grad = torch.ones_like(p)
    state = ops.GuardState(cuda)
    for opt in (torch.optim.AdamW([p], lr=1e-3, fused=True, capturable=True), torch.optim.Adam([p], lr=1e-3)):
        with pytest.raises(RuntimeError, match="gradient guard needs an optimizer segger_adam_step covers"):
            ops.grad_guard(opt, state)
        with pytest.raises(RuntimeError, match="does not cover this optimizer"):
            make_guard(guard_config(clip_grad_norm=1.0), opt, cuda)
    assert guard_config() is None and make_guard(None, None, cuda) is None
    for bad in (dict(clip_grad_norm=0.0), dict(clip_grad_norm=float("nan")), dict(loss_scale=0.0), dict(loss_scale="static")):
        with pytest.raises(ValueError):
            guard_config(**bad)


# ------------------------------------------------------------------------------------------- the captured step
def _step_model(cuda):
    from segger_amd.synthetic import SyntheticSpec
    from tests.test_gpu_train_graph import _model
    return _model(SyntheticSpec(n_tx=5000, n_bd=170, k_tx=7, seed=31), cuda, torch.float32)


def _run_steps(cuda, capture, n_steps=3, hook=None, **guard_kw):
    from segger_amd.train_step_graph import GraphedTrainStep, step_bucket
    m, bg = _step_model(cuda)
    opt = m.configure_optimizers(capturable=True)
    step = GraphedTrainStep(m, opt, step_bucket(bg, granularity=1.3), bg, **guard_kw)
    before = [p.detach().clone() for p in m.parameters()]
    first = None
    for i in range(n_steps):
        step.step(bg, capture=capture)
        if i == 0:
            first = [p.detach().clone() for p in m.parameters()]
    torch.cuda.synchronize()
    return m, opt, step, before, first


@pytest.fixture(scope="module")
def unguarded(cuda):
    """Three steps of the plain step, both routes: computed once, read by the tests below."""
    return {capture: [p.detach().clone() for p in _run_steps(cuda, capture)[0].parameters()] for capture in (False, True)}


@pytest.mark.parametrize("capture", [False, True])
def test_a_loose_guard_at_scale_one_is_the_unguarded_step(cuda, capture, unguarded):
    """``clip_grad_norm`` far above the norm, ``loss_scale=1.0``: ``coef == 1.0f`` exactly, so the guarded update is the
    unguarded one bit for bit.  Two separate runs of the UNGUARDED step are not byte-equal themselves (the loss kernels add
    their gradients with float atomics; see test_gpu_train_graph.py), so the unguarded update is taken on the very gradient
    bytes each guarded step produced -- the plain Adam kernel on a twin of the parameters -- and compared after every one
    of the three steps.  The distance to a separately run unguarded trajectory is printed beside it."""
    from segger_amd import ops
    from segger_amd.train_step_graph import GraphedTrainStep, step_bucket
    m, bg = _step_model(cuda)
    opt = m.configure_optimizers(capturable=True)
    step = GraphedTrainStep(m, opt, step_bucket(bg, granularity=1.3), bg, clip_grad_norm=1e9, loss_scale=1.0)
    group = opt.param_groups[0]
    own = list(group["params"])
    twin = [p.detach().clone().requires_grad_(True) for p in own]
    twin_opt = torch.optim.Adam(twin, lr=group["lr"], betas=group["betas"], eps=group["eps"], capturable=True)
    for i in range(3):
        step.step(bg, capture=capture)
        assert float(step.guard.coef) == 1.0 and int(step.guard.skipped) == 0
        for p, q in zip(own, twin):
            q.grad = None if p.grad is None else p.grad.detach().clone()
        ops.adam_init_state(twin_opt)
        assert ops.adam_step(twin_opt)                                  # the unguarded kernel, the same gradient bytes
        for p, q in zip(own, twin):
            assert torch.equal(p.detach(), q.detach()), i
            if p.grad is not None:
                assert float(opt.state[p]["step"]) == float(twin_opt.state[q]["step"]) == i + 1
                assert torch.equal(opt.state[p]["exp_avg_sq"], twin_opt.state[q]["exp_avg_sq"])
    assert int(step.guard.n_clipped) == 0 and int(step.guard.n_skipped) == 0
    worst = max(float((p.detach() - q).abs().max()) for p, q in zip(m.parameters(), unguarded[capture]))
    print("largest parameter difference to a separately run unguarded trajectory:", worst)


@pytest.mark.parametrize("capture", [False, True])
def test_a_static_loss_scale_leaves_the_trajectory(cuda, capture, unguarded):
    m, opt, step, _, _ = _run_steps(cuda, capture, loss_scale=1024.0)
    assert float(step.guard.scale) == 1024.0 and float(step.guard.coef) == 1.0 / 1024.0 and int(step.guard.n_skipped) == 0
    assert 0.0 < float(step.guard.norm) < 1e3                          # the UNSCALED norm
    for p, q in zip(m.parameters(), unguarded[capture]):
        print("parameter difference, scaled vs unguarded:", float((p.detach() - q).abs().max()))
        assert torch.allclose(p.detach(), q, rtol=2e-2, atol=1e-4)


@pytest.mark.parametrize("capture", [False, True])
def test_a_tiny_clip_norm_clips_every_step(cuda, capture):
    m, opt, step, before, first = _run_steps(cuda, capture, clip_grad_norm=1e-3, loss_scale=8.0)
    g = step.guard
    assert int(g.n_clipped) == 3 and int(g.n_skipped) == 0
    for a, b in zip(before, first):                                     # Adam's first update is at most lr per element
        assert float((a - b).abs().max()) <= 1.01 * m.learning_rate
    assert any(not torch.equal(a, b) for a, b in zip(before, first))
    # the real check: norm and coef of the LAST step against the oracle on that step's own gradients
    grads = [p.grad for grp in opt.param_groups for p in grp["params"] if p.grad is not None]
    want = G.guard_step([x.cpu().numpy() for x in grads], G.fresh_state(8.0, n_clipped=2), G.config(max_norm=1e-3))
    _check_against_oracle(_read(g), want, sum(x.numel() for x in grads))
    assert want["norm"] > 1e-3 and float(g.coef) < 1.0 / 8.0


def test_a_nan_gradient_skips_the_eager_step(cuda):
    from segger_amd.train_step_graph import GraphedTrainStep, step_bucket
    m, bg = _step_model(cuda)
    opt = m.configure_optimizers(capturable=True)
    step = GraphedTrainStep(m, opt, step_bucket(bg, granularity=1.3), bg, skip_nonfinite=True)
    step.step(bg, capture=False)
    leaf, p = next((l, p) for l, p in zip(step._leaves, step._params) if p.grad is not None)
    keep = [q.detach().clone() for q in m.parameters()]
    dropout_counter = int(m.model._step_dev)
    handle = leaf.register_hook(lambda gr: torch.full_like(gr, float("nan")))
    step.step(bg, capture=False)
    handle.remove()
    assert torch.isnan(p.grad).all()
    assert int(step.guard.skipped) == 1 and int(step.guard.n_skipped) == 1 and torch.isnan(step.guard.norm)
    assert all(float(opt.state[q]["step"]) == 1.0 for q in step._params if q.grad is not None)
    assert all(torch.equal(q.detach(), k) for q, k in zip(m.parameters(), keep))
    assert int(m.model._step_dev) == dropout_counter + 256             # the next step draws fresh numbers
    step.step(bg, capture=False)                                       # and training goes on
    assert int(step.guard.skipped) == 0 and float(opt.state[p]["step"]) == 2.0
    assert any(not torch.equal(q.detach(), k) for q, k in zip(m.parameters(), keep))


def test_enable_graphed_training_with_a_guard_logs_norm_and_scale(cuda):
    from segger_amd.synthetic import SyntheticSpec
    from tests.test_gpu_train_graph import _model
    m, bg = _model(SyntheticSpec(n_tx=20000, n_bd=600, k_tx=6, seed=41), cuda, torch.bfloat16)
    twin = copy.deepcopy(m)
    twin.enable_graphed_training(skip_nonfinite=True)
    m.enable_graphed_training(granularity=1.5, clip_grad_norm=1.0, loss_scale="dynamic")
    opt = m.configure_optimizers()

    class Progress:
        ready = completed = 0

    class Wrapper:                                          # the slice of LightningOptimizer the path touches
        def __init__(self, optimizer, prog):
            self.optimizer = optimizer
            self._on_before_step = lambda: setattr(prog, "ready", prog.ready + 1)
            self._on_after_step = lambda: setattr(prog, "completed", prog.completed + 1)
    prog = Progress()
    m.trainer = types.SimpleNamespace(optimizers=[Wrapper(opt, prog)], max_epochs=20, datamodule=None)
    for i in range(3):
        loss = m.training_step(bg, i)
        assert torch.isfinite(loss) and loss.requires_grad is False
        assert torch.isfinite(m.logged["train:grad_norm"]) and float(m.logged["train:grad_norm"]) > 0.0
        assert float(m.logged["train:loss_scale"]) == 65536.0
    assert (prog.ready, prog.completed) == (3, 3)                      # global_step: once per replay
    g = m._graphed_trainer.guard
    assert int(g.n_skipped) == 0 and int(g.growth_tracker) == 3
    assert float(opt.state[next(iter(m.parameters()))]["step"]) == 3.0
    # an optimizer the Adam kernel does not cover: refused with the reason, the guard is not dropped
    with pytest.raises(RuntimeError, match="does not cover this optimizer"):
        twin.trainer = types.SimpleNamespace(optimizers=[torch.optim.AdamW(twin.parameters(), lr=1e-3, capturable=True)], max_epochs=20)
        twin.training_step(bg, 0)
