"""The merged backward launch of one hetero layer (segger_gatv2_bwd_pair: the tx-neighbors-tx source pass and the one-pass
tx-belongs-bd pass in one kernel, one slab-sum launch pair for both edge types) at the shapes where it can go wrong.

The route is the default at every size now, so small shapes reach it -- as far as the library's own route rule lets them:
the merged kernel needs the tx-belongs-bd edge type in wave-per-row mode (at least 32 in-edges per boundary on average,
every transcript in at most one boundary), which no graph of 1, 15, 16 or 17 transcripts can have.  Those transcript counts
are checked all the same (the entry point then runs the edge types one after the other); 4*16+3 and the counts next to a
multiple of 16 above it run the merged kernel with a ragged last source workgroup and a ragged last wave.

Every case runs ``segger_gatv2_bwd_pair`` and the two ``segger_gatv2_bwd`` calls on the same inputs and asserts
  * bit equality of everything the tx-neighbors-tx side writes: grad_xl, grad_xr, grad_pre, grad_att (the sum of its
    destination- and source-pass partials: a source workgroup's partial that differed would show here) and grad_bias;
  * bit equality of the zero fill (the rows of the tx-belongs-bd grad_xl without an out-edge) and of everything the
    tx-belongs-bd side writes.  The single call runs the SAME body at the same rows in flight: the process sets
    SEGGER_BWD_ONE_PASS_IN_PAIR_KERNEL=1, which makes segger_gatv2_bwd launch the merged kernel with an empty source side;
  * the fp64 oracle bounds of tests/test_gpu_gatv2.py / test_gpu_gatv2_grad_att.py for grad_xl, grad_xr, grad_att,
    grad_bias and grad_pre of both sides (grad_pre: one product per entry, scale 4 like grad_xl there).
The switch is read once per process, so all cases run in ONE child process (started with subprocess, this file as its
script), which prints one JSON line per case; the tests below look their case up.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, C = 2, 64
DTYPES = ["float32", "bfloat16", "float16"]
DROPOUTS = ["off", "bits", "eid"]


def _cases():
    """(name, dtype, n_tx, bd_degrees, dropout, gelu, first_tt_source, guard)"""
    out = []
    # the full product of storage type x dropout x GELU on one graph: 163 transcripts (11 source workgroups, the last with
    # 3 rows), boundaries of in-degree 0, 1, 70 (two 64-edge chunks), 45 and 44 -- 5 wave-per-row workgroups, padded to 8
    for dt in DTYPES:
        for dr in DROPOUTS:
            for gelu in (False, True):
                out.append((f"mix-{dt}-{dr}-{'gelu' if gelu else 'lin'}", dt, 163, [0, 1, 70, 45, 44], dr, gelu, 0, False))
    # transcript counts: partial last workgroup / wave.  (1, 15, 16, 17: the two-call route, see the module docstring)
    k = 0
    for n_tx in (1, 15, 16, 17, 4 * 16 + 3, 175, 176, 177):
        for degs in ([n_tx], [0, n_tx - n_tx // 3, 0] if n_tx >= 3 else [0, n_tx, 0], None):
            if degs is None:                               # five boundaries: 0, 1, the rest spread
                if n_tx < 5:
                    continue
                rest = n_tx - 1
                degs = [0, 1, rest // 2, rest - rest // 2 - rest // 4, rest // 4]
            dt, dr = DTYPES[k % 3], DROPOUTS[(k // 3) % 3]
            out.append((f"ntx{n_tx}-nbd{len(degs)}-{dt}-{dr}", dt, n_tx, degs, dr, bool(k % 2), 0, False))
            k += 1
    # one boundary holds all edges, the others none
    for dt in DTYPES:
        out.append((f"one-holds-all-{dt}", dt, 200, [0, 0, 200, 0, 0], "bits", True, 0, False))
    # sources 4..7 of tx-neighbors-tx (the second wave of the first source workgroup) without an out-edge, the other
    # waves of that workgroup with edges: the wave's early exit inside the merged kernel
    for dt in DTYPES:
        out.append((f"edgeless-source-wave-{dt}", dt, 163, [0, 1, 70, 45, 44], "bits", True, 8, False))
    # 3 boundaries -> 3 wave-per-row workgroups padded to 8; 12 -> padded to 16: padded block ids on both sides of the
    # split (the mix graph: 11 source workgroups padded to 16; here 38 padded to 40)
    for dt in DTYPES:
        out.append((f"twelve-boundaries-{dt}", dt, 600, [40 + j for j in range(12)], "eid", False, 0, False))
    # the workspaces at exactly their stated sizes between NaN-filled guards
    for dt in DTYPES:
        out.append((f"exact-workspace-{dt}", dt, 177, [0, 1, 70, 60, 44], "bits", True, 0, True))
    return out


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------------
# the child process
# ---------------------------------------------------------------------------------------------------------------------
def _child():
    import ctypes
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import segger_oracle as oracle
    from segger_amd import _lib, ops
    from segger_amd.graph import build_edge_graph
    from segger_amd.ops.gatv2 import _gat_bwd_args
    from test_gpu_gatv2 import TOL, oracle_conv

    cuda = torch.device("cuda:0")
    lib = _lib.load()
    hc = H * C
    GUARD = 1 << 14

    def err_over_bound(got, ref, dtype, scale):
        atol, rtol = TOL[dtype]
        got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
        if got.numel() == 0:
            return 0.0
        return float(((got - ref).abs() / (scale * (atol + rtol * ref.abs()))).max())

    def one_case(name, dt, n_tx, degs, dropout, gelu, first_src, guard):
        dtype = getattr(torch, dt)
        n_bd = len(degs)
        g = torch.Generator().manual_seed(1000 + n_tx * 7 + n_bd)
        kk = 4
        lo = min(first_src, n_tx - 1)
        ei_tt = torch.stack([torch.randint(lo, n_tx, (n_tx * kk,), generator=g), torch.arange(n_tx).repeat_interleave(kk)])
        if first_src:                                       # sources 0..3 keep edges, 4..first_src-1 have none
            ei_tt[0, : 2 * kk] = torch.arange(4).repeat(2)[: 2 * kk]
        members = torch.randperm(n_tx, generator=g)[: sum(degs)]
        ei_tb = torch.stack([members, torch.repeat_interleave(torch.arange(n_bd), torch.as_tensor(degs))])
        E_tt, E_tb = int(ei_tt.shape[1]), int(ei_tb.shape[1])
        g_tt = build_edge_graph(ei_tt.to(cuda), n_tx, n_tx)
        g_tb = build_edge_graph(ei_tb.to(cuda), n_tx, n_bd, need_by_src="lazy")
        assert g_tb.src_unique()

        xp_tx = torch.randn(n_tx, 3 * hc, generator=g).to(dtype)
        xp_bd = torch.randn(n_bd, hc, generator=g).to(dtype)
        att_tt, bias_tt, att_tb, bias_tb = (torch.randn(hc, generator=g) * s for s in (0.3, 0.1, 0.3, 0.1))
        gy_tx = torch.randn(n_tx, hc, generator=g).to(dtype)
        gy_bd = torch.randn(n_bd, hc, generator=g).to(dtype)
        p = 0.0 if dropout == "off" else 0.2
        seed_tt, seed_tb = 11, 12

        # ---- the fp64 oracle, once per edge type --------------------------------------------------------------------
        def ref(xl, xr, ei, att, bias, gy, seed, E):
            keep = oracle.dropout_keep_mask(seed, E, H, p) if p else None
            o = [t.double().requires_grad_(True) for t in (xl, xr, att, bias)]
            y, pre, _ = oracle_conv(oracle, o[0], o[1], ei, o[2], o[3], H, gelu, keep=keep, p=p)
            pre.retain_grad()
            y.backward(gy.double())
            return [o[0].grad, o[1].grad, o[2].grad, o[3].grad, pre.grad]
        ref_tt = ref(xp_tx[:, :hc], xp_tx[:, hc:2 * hc], ei_tt, att_tt, bias_tt, gy_tx, seed_tt, E_tt)
        ref_tb = ref(xp_tx[:, 2 * hc:], xp_bd, ei_tb, att_tb, bias_tb, gy_bd, seed_tb, E_tb)

        # ---- device: forward once, then the backward both ways -----------------------------------------------------
        d_tx, d_bd = xp_tx.to(cuda), xp_bd.to(cuda)
        dv = [t.to(cuda) for t in (att_tt, bias_tt, att_tb, bias_tb)]
        bits_tt = bits_tb = None
        if dropout == "bits":
            bits_tt = (ops.dropout_bits(g_tt.by_dst, H, p, [seed_tt])[0], ops.dropout_bits(g_tt.by_src, H, p, [seed_tt])[0])
            bits_tb = (ops.dropout_bits(g_tb.by_dst, H, p, [seed_tb])[0], None)
        y_tx, y_bd = torch.empty(n_tx, hc, dtype=dtype, device=cuda), torch.empty(n_bd, hc, dtype=dtype, device=cuda)
        pre_tx, pre_bd = torch.empty_like(y_tx), torch.empty_like(y_bd)
        lse_tx, lse_bd = torch.empty(n_tx, H, device=cuda), torch.empty(n_bd, H, device=cuda)
        ops.gatv2_fwd_launch(g_tt.by_dst, d_tx[:, :hc], d_tx[:, hc:2 * hc], dv[0], dv[1], H, C, y_tx, pre=pre_tx, lse=lse_tx,
                             apply_gelu=gelu, dropout_p=p, seed=seed_tt, keep_bits=None if bits_tt is None else bits_tt[0])
        ops.gatv2_fwd_launch(g_tb.by_dst, d_tx[:, 2 * hc:], d_bd, dv[2], dv[3], H, C, y_bd, pre=pre_bd, lse=lse_bd,
                             apply_gelu=gelu, dropout_p=p, seed=seed_tb, keep_bits=None if bits_tb is None else bits_tb[0])
        saved_tx, saved_bd = (pre_tx, pre_bd) if gelu else (y_tx, y_bd)

        def backward(merged):
            nan = float("nan")
            gxp_tx = torch.full((n_tx, 3 * hc), nan, dtype=dtype, device=cuda)
            gxp_bd = torch.full((n_bd, hc), nan, dtype=dtype, device=cuda)
            gp_tx, gp_bd = torch.full_like(y_tx, nan), torch.full_like(y_bd, nan)
            ds_tx, ds_bd = torch.empty(n_tx, H, 2, device=cuda), torch.empty(n_bd, H, 2, device=cuda)
            kw = dict(apply_gelu=gelu, dropout_p=p)
            a, par_a, keep_a, zeroed = _gat_bwd_args(
                g_tt, d_tx[:, :hc], d_tx[:, hc:2 * hc], dv[0], dv[1], H, C, gy_tx.to(cuda), saved_tx, lse_tx, gxp_tx[:, :hc],
                gxp_tx[:, hc:2 * hc], seed=seed_tt, keep_bits=bits_tt, zero_rows_out=gxp_tx[:, 2 * hc:] if merged else None,
                scratch=(gp_tx, ds_tx), **kw)
            b, par_b, keep_b, _ = _gat_bwd_args(
                g_tb, d_tx[:, 2 * hc:], d_bd, dv[2], dv[3], H, C, gy_bd.to(cuda), saved_bd, lse_bd, gxp_tx[:, 2 * hc:], gxp_bd,
                seed=seed_tb, keep_bits=bits_tb, grad_xl_zeroed=zeroed if merged else False, scratch=(gp_bd, ds_bd), **kw)
            assert b.src_unique and not a.src_unique
            bufs = []
            if guard:                                       # each side's workspace at exactly its stated size
                stated = (lib.segger_gatv2_bwd_workspace_bytes_two_pass(n_tx, n_tx, E_tt, H, C),
                          lib.segger_gatv2_bwd_workspace_bytes(n_bd, H, C))
                for args, size in zip((a, b), stated):
                    buf = torch.full((GUARD + size + GUARD,), 0xFF, dtype=torch.uint8, device=cuda)   # fp32 NaN throughout
                    args.workspace, args.workspace_bytes = buf.data_ptr() + GUARD, size
                    bufs.append((buf, size))
            with _lib.on_device(cuda):
                if merged:
                    rc = lib.segger_gatv2_bwd_pair(ctypes.byref(a), ctypes.byref(b), _lib.stream_ptr(cuda))
                else:
                    rc = lib.segger_gatv2_bwd(ctypes.byref(a), _lib.stream_ptr(cuda)) or \
                         lib.segger_gatv2_bwd(ctypes.byref(b), _lib.stream_ptr(cuda))
            _lib.check(rc, "segger_gatv2_bwd[_pair]")
            torch.cuda.synchronize()
            for buf, size in bufs:
                assert bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + size:] == 0xFF).all()), "guard overwritten"
            return {"tt": [gxp_tx[:, :hc], gxp_tx[:, hc:2 * hc], par_a[0], par_a[1], gp_tx],
                    "tb": [gxp_tx[:, 2 * hc:], gxp_bd, par_b[0], par_b[1], gp_bd]}

        m, s = backward(True), backward(False)
        names = ["grad_xl", "grad_xr", "grad_att", "grad_bias", "grad_pre"]
        figures, bad = {}, []
        for side in ("tt", "tb"):
            for nm, x, y in zip(names, m[side], s[side]):
                if not bool(torch.isfinite(x.float()).all()):
                    bad.append(f"{side}.{nm}: not finite")
                if not torch.equal(x, y):
                    bad.append(f"{side}.{nm}: merged != single calls, max diff {float((x.float() - y.float()).abs().max()):.3e}")
        deg_in_tt, deg_out_tt = kk, int(torch.bincount(ei_tt[0], minlength=n_tx).max())
        scales = {"tt": [4.0 * max(1.0, deg_out_tt) ** 0.5, 4.0 * deg_in_tt ** 0.5, 4.0 * max(1.0, E_tt) ** 0.5,
                         4.0 * n_tx ** 0.5, 4.0],
                  "tb": [4.0, 4.0 * max(1.0, max(degs)) ** 0.5, 4.0 * max(1.0, E_tb) ** 0.5, 4.0 * n_bd ** 0.5, 4.0]}
        for side, refs in (("tt", ref_tt), ("tb", ref_tb)):
            for nm, x, r, sc in zip(names, m[side], refs, scales[side]):
                f = err_over_bound(x, r, dtype, sc)
                figures[f"{side}.{nm}"] = round(f, 4)
                if not f <= 1.0:
                    bad.append(f"{side}.{nm}: error / oracle bound = {f:.3f}")
        wpr = E_tb / n_bd >= 32.0
        return {"name": name, "bad": bad, "err_over_bound": figures, "merged_route": bool(wpr and n_tx > 0)}

    for case in CASES:
        try:
            r = one_case(*case)
        except Exception as e:  # noqa: BLE001
            r = {"name": case[0], "bad": [f"{type(e).__name__}: {e}"], "err_over_bound": {}, "merged_route": None}
        print("CASE " + json.dumps(r), flush=True)


if __name__ == "__main__":
    _child()
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def results(cuda):
    env = dict(os.environ, SEGGER_BWD_ONE_PASS_IN_PAIR_KERNEL="1")
    env.pop("SEGGER_BWD_PAIR_MAX_ROWS", None)                # the default route: merged at every size
    run = subprocess.run([sys.executable, "-s", os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    out = {}
    for ln in run.stdout.splitlines():
        if ln.startswith("CASE "):
            r = json.loads(ln[5:])
            out[r["name"]] = r
    assert run.returncode == 0 and len(out) == len(CASES), f"child exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_merged_launch_equals_single_calls_and_the_oracle(results, name):
    r = results[name]
    print(name, "merged kernel" if r["merged_route"] else "two-call route", r["err_over_bound"])
    assert not r["bad"], r["bad"]


@pytest.mark.gpu
def test_the_shapes_reach_the_merged_kernel(results):
    """The route rule as the cases' graphs meet it: everything but the 1..17-transcript graphs (and 67 transcripts split
    over five boundaries) has its tx-belongs-bd edge type in wave-per-row mode."""
    merged = {c[0] for c in CASES if results[c[0]]["merged_route"]}
    assert all(n in merged for n in [c[0] for c in CASES if c[0].startswith(("mix-", "one-holds", "edgeless", "twelve", "exact"))])
    assert {f"ntx{n}-nbd1-" in " ".join(merged) for n in (67, 175, 176, 177)} == {True}
    assert not any(n.startswith(("ntx1-", "ntx15-", "ntx16-", "ntx17-")) for n in merged)
