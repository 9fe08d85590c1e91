"""The gradient guard's float64 oracle (tests/grad_guard_cases.py, CPU): held to its hand-worked cases, and on clean steps
to what it stands in for -- ``torch.nn.utils.clip_grad_norm_`` on the unscaled gradients and the recurrence of
``torch.amp.GradScaler.update`` (torch/amp/grad_scaler.py: ``_amp_update_scale_``)."""
import math

import numpy as np
import pytest
import torch

from tests import grad_guard_cases as G


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_oracle_gives_the_hand_worked_numbers(case):
    _, grads, state, cfg, want = case
    got = G.guard_step([np.asarray(g, dtype=np.float32) for g in grads], state, cfg)
    assert set(got) == set(want)
    for k in ("skip", "growth_tracker", "n_skipped", "n_clipped"):
        assert got[k] == want[k], k
    for k in ("coef", "scale"):
        assert got[k].dtype == np.float32 and got[k] == want[k], (k, got[k], want[k])
    if want["skip"]:
        assert math.isnan(got["norm"])
    else:
        assert got["norm"] == pytest.approx(want["norm"], rel=1e-15, abs=0.0)


def test_growth_happens_on_the_interval_and_a_skip_restarts_the_count():
    cfg = G.config(max_norm=1.0, growth_interval=3)
    st = G.fresh_state(8.0)
    clean, bad = [np.array([0.25, 0.5], dtype=np.float32)], [np.array([0.25, np.inf], dtype=np.float32)]
    seen = []
    for g in (clean, clean, bad, clean, clean, clean, clean):
        r = G.guard_step(g, st, cfg)
        st = G.next_state(r)
        seen.append((float(st["scale"]), st["growth_tracker"], r["skip"]))
    assert seen == [(8.0, 1, 0), (8.0, 2, 0), (4.0, 0, 1), (4.0, 1, 0), (4.0, 2, 0), (8.0, 0, 0), (8.0, 1, 0)]
    assert (st["n_skipped"], st["n_clipped"]) == (1, 0)


def _torch_scaler_update(scale, tracker, found_inf, growth, backoff, interval):
    """GradScaler.update's recurrence on float32 / int32 CPU tensors, as aten's amp_update_scale kernel writes it."""
    scale, tracker = torch.tensor(scale, dtype=torch.float32), torch.tensor(tracker, dtype=torch.int32)
    if found_inf:
        scale, tracker = scale * backoff, torch.zeros_like(tracker)
    else:
        tracker = tracker + 1
        if int(tracker) == interval:
            scale, tracker = scale * growth, torch.zeros_like(tracker)
    return float(scale), int(tracker)


@pytest.mark.parametrize("max_norm", [0.05, 1.0, 1e6])
def test_clean_steps_match_torch_clipping_and_scaler_recurrence(max_norm):
    gen = torch.Generator().manual_seed(11)
    shapes = [(37, 5), (129,), (1,), (0,), (2049,)]
    cfg = G.config(max_norm=max_norm, growth_interval=2)
    st = G.fresh_state(1024.0)
    t_scale, t_tracker = 1024.0, 0
    for step in range(5):
        true = [torch.randn(s, generator=gen) * 10.0 ** (step % 3 - 1) for s in shapes]
        scaled = [g * float(st["scale"]) for g in true]                       # a power of two: exact
        r = G.guard_step([g.numpy() for g in scaled], st, cfg)
        ps = [torch.zeros(s, requires_grad=True) for s in shapes]
        for p, g in zip(ps, true):
            p.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)                   # fp32 throughout
        assert r["skip"] == 0 and r["norm"] == pytest.approx(float(norm), rel=1e-5)
        for p, g in zip(ps, scaled):                                          # what the guarded Adam sees: g * coef
            assert torch.allclose(g * float(r["coef"]), p.grad, rtol=1e-5, atol=0.0)
        assert r["n_clipped"] - st["n_clipped"] == int(float(norm) + 1e-6 > max_norm)
        t_scale, t_tracker = _torch_scaler_update(t_scale, t_tracker, False, cfg["growth"], cfg["backoff"], cfg["growth_interval"])
        st = G.next_state(r)
        assert (float(st["scale"]), st["growth_tracker"]) == (t_scale, t_tracker)
    assert float(st["scale"]) == 4096.0                                       # grew after steps 2 and 4


def test_a_skipped_step_matches_the_scaler_recurrence():
    st = G.fresh_state(65536.0, growth_tracker=1999)
    r = G.guard_step([np.array([1.0, np.nan], dtype=np.float32)], st, G.config(growth_interval=2000))
    assert (float(r["scale"]), r["growth_tracker"]) == _torch_scaler_update(65536.0, 1999, True, 2.0, 0.5, 2000) == (32768.0, 0)
