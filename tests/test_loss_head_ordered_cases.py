"""The float64 oracle of the ordered loss-head backward (tests/loss_head_ordered_cases.py) against plain torch autograd of
the three losses (CPU): hand-worked cases first, then small random instances that hold every special case -- skipped
triplets, a zero weight, padded segmentation triplets, a transcript without a segmentation triplet, a boundary without
transcripts, rows on both sides of the 64-term threshold between the serial and the 16-partial-sum form."""
import numpy as np
import pytest
import torch

import loss_head_ordered_cases as lc


def torch_reference(p, gout):
    """out [4] and the gradients of (y_tx or z_tx, z_bd) by autograd, float64, vectorised: no order in common with the oracle"""
    t = lambda v: torch.tensor(np.asarray(v))
    leaf_tx = t(p["y_tx"] if p["y_tx"] is not None else p["z_tx"]).requires_grad_(True)
    zbd = t(p["z_bd"]).requires_grad_(True)
    ztx = leaf_tx / leaf_tx.norm(dim=1, keepdim=True).clamp(min=p["norm_eps"]) if p["y_tx"] is not None else leaf_tx
    n_tx, n_bd, n_sg = len(ztx), len(zbd), len(p["sg_src"])
    pos, neg = t(p["tx_pos"]), t(p["tx_neg"])
    ok = (pos >= 0) & (neg >= 0)
    a_ = ztx[ok]
    d = lambda x, y, eps: (x - y + eps).norm(dim=1)
    l_tx = (d(a_, ztx[pos[ok]], p["tx_eps"]) - d(a_, ztx[neg[ok]], p["tx_eps"]) + p["tx_margin"]).clamp(min=0).sum() / n_tx
    bp, bn, w = t(p["bd_pos"]), t(p["bd_neg"]), t(p["bd_w"])
    cos = lambda x, y: (x * y).sum(1) / (x.norm(dim=1).clamp(min=p["bd_eps"]) * y.norm(dim=1).clamp(min=p["bd_eps"]))
    l_bd = (w * ((cos(zbd, zbd[bp]) - (1 - t(p["bd_dpos"]))) ** 2 + (cos(zbd, zbd[bn]) - (1 - t(p["bd_dneg"]))) ** 2)).sum()
    l_sg = torch.zeros((), dtype=torch.float64)
    if n_sg:
        src, sp, sn = t(p["sg_src"]), t(p["sg_pos"]), t(p["sg_neg"])
        ok = (sp >= 0) & (sn >= 0)
        a_, pj, nv = ztx[src[ok]], zbd[sp[ok]], zbd[sn[ok]]
        if p["sg_kind"] == "bce":
            sp_ = torch.nn.functional.softplus
            l_sg = (sp_(-(a_ * pj).sum(1)).sum() + sp_((a_ * nv).sum(1)).sum()) / (2 * n_sg)
        else:
            l_sg = (d(a_, pj, p["sg_eps"]) - d(a_, nv, p["sg_eps"]) + p["sg_margin"]).clamp(min=0).sum() / n_sg
    out3 = torch.stack([l_tx, l_bd, l_sg]) * t(p["a"])
    out = torch.cat([out3, (out3 * t(p["b"])).sum().reshape(1)])
    out.backward(t(gout))
    return out.detach().numpy(), leaf_tx.grad.numpy(), zbd.grad.numpy()


def test_one_triplet_by_hand():
    """Two transcripts on the unit circle, one boundary: loss_tx's only active triplet is (0; 1, 1) -> no loss (same
    distance), so take (0; pos 1, neg 0): d(0,1) = sqrt(2), d(0,0) = |eps| ~ 0 -> hinge sqrt(2) + m active."""
    p = lc.problem(n_tx=2, n_bd=1, n_sg=0, C=2, seed=1)
    p["z_tx"] = np.array([[1.0, 0.0], [0.0, 1.0]])
    p["tx_pos"], p["tx_neg"] = np.array([1, -1]), np.array([0, -1])
    p["tx_eps"], p["tx_margin"] = 0.0, 0.5
    p["a"], p["b"] = np.ones(3), np.array([1.0, 0.0, 0.0])
    p["bd_w"][:] = 0.0
    out = lc.losses(p)
    assert out[0] == pytest.approx((np.sqrt(2) + 0.5) / 2) and out[3] == out[0] and out[1] == out[2] == 0
    gtx, gbd = lc.gradients(p, np.array([0.0, 0.0, 0.0, 1.0]))
    # d/d z0 of |z0 - z1| / 2 = (1, -1) / sqrt(2) / 2; the negative is the anchor itself at distance 0: weight 0
    assert np.allclose(gtx[0], np.array([1.0, -1.0]) / np.sqrt(2) / 2) and np.allclose(gtx[1], -gtx[0])
    assert not gbd.any()


def test_metric_pair_by_hand():
    """Two boundaries at right angles naming each other: cos = 0, target 1 - d = 0.5 -> r = -0.5 for all four terms."""
    p = lc.problem(n_tx=2, n_bd=2, n_sg=0, C=2, seed=2)
    p["z_bd"] = np.array([[1.0, 0.0], [0.0, 1.0]])
    p["bd_pos"], p["bd_neg"] = np.array([1, 0]), np.array([1, 0])
    p["bd_dpos"][:], p["bd_dneg"][:], p["bd_w"][:] = 0.5, 0.5, 1.0
    p["tx_pos"][:] = -1
    p["sg_src"] = p["sg_pos"] = p["sg_neg"] = np.zeros(0, np.int64)
    p["a"], p["b"] = np.ones(3), np.array([0.0, 1.0, 0.0])
    assert lc.losses(p)[1] == pytest.approx(4 * 0.25)
    _, gbd = lc.gradients(p, np.array([0.0, 0.0, 0.0, 1.0]))
    # row 0: own two terms 2 * (-0.5) * z1 each, plus the same from row 1's two terms naming it: d cos / d z0 = z1
    assert np.allclose(gbd, np.array([[0.0, -4.0], [-4.0, 0.0]]))


CASES = [dict(seed=3), dict(seed=4, sg_kind="bce"), dict(seed=5, prenorm=True), dict(seed=6, n_bd=1), dict(seed=7, n_bd=2),
         dict(seed=8, n_tx=300, n_bd=7, n_sg=200, hot=((2, 63, 0), (3, 64, 1), (4, 65, 0), (5, 100, 1))),
         dict(seed=9, n_tx=300, n_bd=7, n_sg=200, sg_kind="bce", prenorm=True, hot=((2, 40, 0), (2, 40, 1)))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items() if k != "hot"))
def test_oracle_equals_autograd(case):
    p = lc.problem(**case)
    if case.get("n_tx") == 300:                     # one boundary draws every sampled negative
        p["sg_neg"][p["sg_neg"] >= 0] = 6
    gout = np.array([1.0, 0.0, 0.5, 1.7])
    out, gtx, gbd = torch_reference(p, gout)
    assert np.allclose(lc.losses(p), out, rtol=1e-12, atol=1e-14)
    otx, obd = lc.gradients(p, gout)
    assert np.abs(otx).max() > 0 and np.abs(obd).max() > 0
    assert np.allclose(otx, gtx, rtol=1e-10, atol=1e-13), np.abs(otx - gtx).max()
    assert np.allclose(obd, gbd, rtol=1e-10, atol=1e-13), np.abs(obd - gbd).max()


def test_long_lists_are_summed_as_sixteen_interleaved_partials():
    """The partial sums are visible in the bits: 17 terms of a long list land as P[0] = t0 + t16, P[1] = t1, ..."""
    terms = [np.array([10.0 ** -k]) for k in range(17)]
    got = lc._team_sum(np.array([1.0]), [terms])
    want = np.array([1.0])
    part = [terms[0] + terms[16]] + terms[1:16]
    for q in part:
        want = want + q
    assert got == want


# ------------------------------------------------------------------------------------------------- the model's surface
def _lit():
    from segger_amd import LitISTEncoder
    return LitISTEncoder(n_genes=20, in_channels=32, hidden_channels=16, out_channels=16, n_heads=2)


def test_the_keyword_and_the_environment_switch_reach_the_trainer(monkeypatch):
    """``enable_graphed_training(deterministic=)``, ``fast(deterministic=)`` and ``SEGGER_AMD_DETERMINISTIC=1``: the flag is
    kept on the module (the fused eager path reads it) and handed to the ``GraphedTrainer``; off by default, and then not
    in the trainer's keywords at all."""
    for name in ("SEGGER_AMD_DETERMINISTIC", "SEGGER_AMD_FAST", "SEGGER_AMD_GRAPHED"):
        monkeypatch.delenv(name, raising=False)
    m = _lit()
    assert m.deterministic is False and m._graphed_kw is None
    m.enable_graphed_training(granularity=1.5)
    assert m.deterministic is False and m._graphed_kw == dict(granularity=1.5)
    m.enable_graphed_training(deterministic=True)
    assert m.deterministic is True and m._graphed_kw == dict(deterministic=True)
    m.enable_graphed_training(deterministic=False)
    assert m.deterministic is False and m._graphed_kw == {}
    m.fast(deterministic=True, clip_grad_norm=1.0)
    assert m.deterministic and m._graphed_kw["deterministic"] is True and m._graphed_kw["clip_grad_norm"] == 1.0
    monkeypatch.setenv("SEGGER_AMD_DETERMINISTIC", "1")
    m = _lit()
    assert m.deterministic is True and m._graphed_kw is None            # eager, fused loss head: ordered
    assert m.enable_graphed_training()._graphed_kw == dict(deterministic=True)
    monkeypatch.setenv("SEGGER_AMD_GRAPHED", "1")
    assert _lit()._graphed_kw == dict(deterministic=True)
    monkeypatch.setenv("SEGGER_AMD_FAST", "1")
    assert _lit()._graphed_kw == dict(deterministic=True)
    import inspect
    from segger_amd.train_step_graph import GraphedTrainStep, GraphedTrainer
    for cls in (GraphedTrainStep, GraphedTrainer):
        assert inspect.signature(cls.__init__).parameters["deterministic"].default is False
