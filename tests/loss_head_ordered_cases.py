"""The float64 oracle of the loss head's ORDERED backward (segger_loss_head_ordered_fwd / _bwd, include/segger_amd.h):
the three losses, their weighted total and the two gradient matrices, every sum taken in the order the header documents --
plain numpy, one term at a time.  Shared by the CPU test that pins it to torch autograd on hand-worked cases
(tests/test_loss_head_ordered_cases.py) and by the GPU tests of the kernels (tests/test_gpu_loss_head_ordered.py)."""
import numpy as np

SERIAL_CAP = 64          # contributions a transcript row adds one after the other (csrc/loss_head_ordered.hip kSerialCap)
TEAM = 16                # partial sums of a longer row, and of every boundary row (kTeam)


def _softplus(x):
    return max(x, 0.0) + np.log1p(np.exp(-abs(x)))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def losses(p):
    """-> float64 [4]: (a0 loss_tx, a1 loss_bd, a2 loss_sg, sum_i b_i out_i)."""
    ztx, zbd = p["z_tx"], p["z_bd"]
    n_tx, n_bd, n_sg = len(ztx), len(zbd), len(p["sg_src"])
    l_tx = 0.0
    for t in range(n_tx):
        ip, i_n = p["tx_pos"][t], p["tx_neg"][t]
        if 0 <= ip < n_tx and 0 <= i_n < n_tx:
            dap = np.linalg.norm(ztx[t] - ztx[ip] + p["tx_eps"])
            dan = np.linalg.norm(ztx[t] - ztx[i_n] + p["tx_eps"])
            l_tx += max(dap - dan + p["tx_margin"], 0.0)
    l_bd = 0.0
    for i in range(n_bd):
        ip, i_n, w = p["bd_pos"][i], p["bd_neg"][i], p["bd_w"][i]
        if 0 <= ip < n_bd and 0 <= i_n < n_bd and w != 0:
            cx = max(np.linalg.norm(zbd[i]), p["bd_eps"])
            for q, d in ((ip, p["bd_dpos"][i]), (i_n, p["bd_dneg"][i])):
                cq = max(np.linalg.norm(zbd[q]), p["bd_eps"])
                l_bd += w * (zbd[i] @ zbd[q] / (cx * cq) - (1.0 - d)) ** 2
    l_sg = 0.0
    for e in range(n_sg):
        ia, ip, i_n = p["sg_src"][e], p["sg_pos"][e], p["sg_neg"][e]
        if 0 <= ia < n_tx and 0 <= ip < n_bd and 0 <= i_n < n_bd:
            if p["sg_kind"] == "bce":
                l_sg += _softplus(-(ztx[ia] @ zbd[ip])) + _softplus(ztx[ia] @ zbd[i_n])
            else:
                l_sg += max(np.linalg.norm(ztx[ia] - zbd[ip] + p["sg_eps"]) - np.linalg.norm(ztx[ia] - zbd[i_n] + p["sg_eps"])
                            + p["sg_margin"], 0.0)
    raw = np.array([l_tx / n_tx if n_tx else 0.0, l_bd,
                    l_sg * (0.5 if p["sg_kind"] == "bce" else 1.0) / n_sg if n_sg else 0.0])
    out = raw * p["a"]
    return np.append(out, out @ p["b"])


def _team_sum(start, terms):
    """start + P[0] + ... + P[15], term k added to P[k mod 16] in list order (several lists: k restarts in each)."""
    part = [np.zeros_like(start) for _ in range(TEAM)]
    for lst in terms:
        for k, t in enumerate(lst):
            part[k % TEAM] = part[k % TEAM] + t
    g = start.copy()
    for q in range(TEAM):
        g = g + part[q]
    return g


def gradients(p, gout):
    """-> (grad_tx [n_tx, C], grad_bd [n_bd, C]) float64 for the incoming gradient ``gout`` [4], in the documented order;
    with ``p["y_tx"]`` (z_tx = y_tx / max(|y_tx|, norm_eps) row-wise) grad_tx is the gradient of y_tx."""
    ztx, zbd = p["z_tx"], p["z_bd"]
    n_tx, n_bd, n_sg = len(ztx), len(zbd), len(p["sg_src"])
    C = ztx.shape[1]
    bce = p["sg_kind"] == "bce"
    graw = (gout[3] * p["b"] + gout[:3]) * p["a"]
    sc_tx = graw[0] / n_tx if n_tx else 0.0
    sc_bd = graw[1]
    sc_sg = graw[2] * (0.5 if bce else 1.0) / n_sg if n_sg else 0.0

    # ---- loss_tx: which triplets are active, and their reciprocal distances
    w_tx = np.zeros((n_tx, 2))
    for t in range(n_tx):
        ip, i_n = p["tx_pos"][t], p["tx_neg"][t]
        if 0 <= ip < n_tx and 0 <= i_n < n_tx:
            dap = np.linalg.norm(ztx[t] - ztx[ip] + p["tx_eps"])
            dan = np.linalg.norm(ztx[t] - ztx[i_n] + p["tx_eps"])
            if dap - dan + p["tx_margin"] > 0:
                w_tx[t] = (1.0 / dap if dap > 0 else 0.0, 1.0 / dan if dan > 0 else 0.0)
    as_pos = [[] for _ in range(n_tx)]                 # ascending triplet id by construction
    as_neg = [[] for _ in range(n_tx)]
    for t in range(n_tx):
        if w_tx[t, 0] != 0:
            as_pos[p["tx_pos"][t]].append(t)
        if w_tx[t, 1] != 0:
            as_neg[p["tx_neg"][t]].append(t)
    sg_of_tx = np.full(n_tx, -1)
    sg_ok = np.zeros(n_sg, bool)
    for e in range(n_sg):
        ia, ip, i_n = p["sg_src"][e], p["sg_pos"][e], p["sg_neg"][e]
        sg_ok[e] = 0 <= ia < n_tx and 0 <= ip < n_bd and 0 <= i_n < n_bd
        if 0 <= ia < n_tx:
            assert sg_of_tx[ia] < 0, "a transcript anchors two segmentation triplets: not this route's case"
            sg_of_tx[ia] = e

    def sg_terms(e):
        """(anchor term, positive row's term, negative row's term) of segmentation triplet e, or None when it adds nothing"""
        a_, pj, nv = ztx[p["sg_src"][e]], zbd[p["sg_pos"][e]], zbd[p["sg_neg"][e]]
        if bce:
            dlp, dln = (_sigmoid(a_ @ pj) - 1.0) * sc_sg, _sigmoid(a_ @ nv) * sc_sg
            return dlp * pj + dln * nv, dlp * a_, dln * a_
        dp, dn = a_ - pj + p["sg_eps"], a_ - nv + p["sg_eps"]
        dap, dan = np.linalg.norm(dp), np.linalg.norm(dn)
        if dap - dan + p["sg_margin"] <= 0:
            return None
        ip_, in_ = (sc_sg / dap if dap > 0 else 0.0), (sc_sg / dan if dan > 0 else 0.0)
        return dp * ip_ - dn * in_, -dp * ip_, dn * in_

    gtx = np.zeros((n_tx, C))
    for r in range(n_tx):
        g = np.zeros(C)
        if w_tx[r].any():                                                                   # (1)
            g = g + ((ztx[r] - ztx[p["tx_pos"][r]] + p["tx_eps"]) * (w_tx[r, 0] * sc_tx)
                     - (ztx[r] - ztx[p["tx_neg"][r]] + p["tx_eps"]) * (w_tx[r, 1] * sc_tx))
        terms = [-(ztx[t] - ztx[r] + p["tx_eps"]) * (w_tx[t, 0] * sc_tx) for t in as_pos[r]]        # (2)
        terms += [(ztx[t] - ztx[r] + p["tx_eps"]) * (w_tx[t, 1] * sc_tx) for t in as_neg[r]]        # (3)
        if len(terms) <= SERIAL_CAP:
            for t in terms:
                g = g + t
        else:
            g = _team_sum(g, [terms])
        e = sg_of_tx[r]
        if e >= 0 and sg_ok[e] and sc_sg != 0:                                              # (4)
            st = sg_terms(e)
            if st is not None:
                g = g + st[0]
        if p.get("y_tx") is not None:
            y = p["y_tx"][r]
            nrm = np.linalg.norm(y)
            inv = 1.0 / max(nrm, p["norm_eps"])
            dot = (y * inv) @ g if nrm >= p["norm_eps"] else 0.0
            g = (g - y * inv * dot) * inv
        gtx[r] = g

    # ---- boundary rows
    def bd_coef(i, q, d):
        """loss_bd node i against row q with target d -> (cos, g, 1 / (cx cq))"""
        cx, cq = max(np.linalg.norm(zbd[i]), p["bd_eps"]), max(np.linalg.norm(zbd[q]), p["bd_eps"])
        cosv = zbd[i] @ zbd[q] / (cx * cq)
        return cosv, 2.0 * p["bd_w"][i] * (cosv - (1.0 - d)) * sc_bd, 1.0 / (cx * cq)

    bd_ok = [0 <= p["bd_pos"][i] < n_bd and 0 <= p["bd_neg"][i] < n_bd and p["bd_w"][i] != 0 for i in range(n_bd)]
    gbd = np.zeros((n_bd, C))
    for j in range(n_bd):
        g = np.zeros(C)
        x, sjj = zbd[j], zbd[j] @ zbd[j]
        live = np.sqrt(sjj) > p["bd_eps"]
        if bd_ok[j]:                                                                        # (1)
            ip, i_n = p["bd_pos"][j], p["bd_neg"][j]
            cp, gp, rp = bd_coef(j, ip, p["bd_dpos"][j])
            cn, gn, rn = bd_coef(j, i_n, p["bd_dneg"][j])
            ax = (gp * cp + gn * cn) / sjj if live else 0.0
            g = gp * rp * zbd[ip] + gn * rn * zbd[i_n] - ax * x
        seg = []
        for role, idx, dd in ((0, p["bd_pos"], p["bd_dpos"]), (1, p["bd_neg"], p["bd_dneg"])):       # (2), (3)
            for i in range(n_bd):
                if bd_ok[i] and idx[i] == j:
                    cq, gq, rq = bd_coef(i, j, dd[i])
                    seg.append(gq * rq * zbd[i] - (gq * cq / sjj if live else 0.0) * x)
        for e in range(n_sg):                                                               # (4)
            if sg_ok[e] and p["sg_neg"][e] == j:
                st = sg_terms(e)
                if st is not None:
                    seg.append(st[2])
        own = []
        for s in range(p["sg_indptr"][j], p["sg_indptr"][j + 1]) if n_sg else ():           # (5)
            e = p["sg_eid"][s]
            if sg_ok[e] and p["sg_pos"][e] == j:
                st = sg_terms(e)
                if st is not None:
                    own.append(st[1])
        gbd[j] = _team_sum(g, [seg, own])
    return gtx, gbd


def groups_by_positive(sg_pos, n_bd):
    """(indptr [n_bd + 1], eid) of the segmentation triplets grouped by positive row, stable (skipped ones, pos < 0, under
    row 0 as the encoder's by-destination view of clamped indices has them)."""
    key = np.clip(np.asarray(sg_pos), 0, None)
    eid = np.argsort(key, kind="stable")
    indptr = np.zeros(n_bd + 1, np.int64)
    np.add.at(indptr, key + 1, 1)
    return np.cumsum(indptr), eid.astype(np.int32)


def problem(n_tx=40, n_bd=5, n_sg=24, C=8, sg_kind="triplet", seed=0, prenorm=False, hot=(), tx_margin=0.3):
    """A small random instance with every special case in it: skipped loss_tx triplets (-1), a zero loss_bd weight, padded
    segmentation triplets (-1), a transcript without a segmentation triplet, a boundary without transcripts (the last).
    ``hot``: (row, count, as_negative) triples, rows below 8 -- exactly `count` triplets name `row` (no random draw names a
    row below 8 then, and none of those triplets is skipped; with ``tx_margin`` above 2 every one of them is active on unit
    rows, so that `count` is the number of contributions the row receives)."""
    g = np.random.default_rng(seed)
    y = g.standard_normal((n_tx, C))
    zbd = g.standard_normal((n_bd, C))
    zbd /= np.linalg.norm(zbd, axis=1, keepdims=True)
    p = dict(z_tx=y / np.linalg.norm(y, axis=1, keepdims=True), z_bd=zbd, y_tx=y if prenorm else None, norm_eps=1e-12,
             tx_pos=g.integers(8 if hot else 0, n_tx, n_tx), tx_neg=g.integers(8 if hot else 0, n_tx, n_tx),
             tx_margin=tx_margin, tx_eps=1e-6,
             bd_pos=g.integers(0, n_bd, n_bd), bd_neg=g.integers(0, n_bd, n_bd), bd_dpos=g.random(n_bd), bd_dneg=g.random(n_bd),
             bd_w=np.full(n_bd, 1.0 / n_bd), bd_eps=1e-8, sg_kind=sg_kind, sg_margin=0.4, sg_eps=1e-6,
             a=np.array([1.3, 1.0, 0.7]), b=np.array([0.5, 0.2, 0.3]))
    at = [8 if hot else 0] * 2                                          # the positives' and the negatives' side fill apart
    for row, count, as_neg in hot:
        assert row < 8
        (p["tx_neg"] if as_neg else p["tx_pos"])[at[as_neg]:at[as_neg] + count] = row
        at[as_neg] += count
    assert max(at) <= n_tx
    p["tx_pos"][max(at)::7] = -1
    if n_bd > 3:
        p["bd_w"][3] = 0.0
    n_sg = min(n_sg, n_tx - 1) if n_bd > 1 else 0
    p["sg_src"] = g.permutation(n_tx - 1)[:n_sg]                       # the last transcript anchors none
    hi = max(n_bd - 1, 1)                                              # the last boundary has no transcripts
    p["sg_pos"] = g.integers(0, hi, n_sg)
    p["sg_neg"] = (p["sg_pos"] + g.integers(1, max(n_bd, 2), n_sg)) % max(n_bd, 1)
    if n_sg > 4:
        p["sg_pos"][-2:] = -1
        p["sg_neg"][-2:] = -1
    p["sg_indptr"], p["sg_eid"] = groups_by_positive(p["sg_pos"], n_bd)
    return p
