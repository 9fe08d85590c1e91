"""grad_att of the fused GATv2 backward on the graphs where a per-row formulation can go wrong.

The two-pass backward forms grad_att from per-row sums: per destination x_r * (c1 Sde + c2 Sg) in the destination pass,
per source x_l * (c1 Sde + c2 Sg) in the source pass, each pass leaving one partial per workgroup that one deterministic
sum adds up.  What can break is therefore a row or a workgroup that is skipped or counted twice (edgeless rows, a source
wave that leaves early, rows past the end of a ragged last workgroup, the groups of a wave that share one row), a sign at
t = +-0, or a dropped edge that still counts.  Every case compares grad_att first and grad_xl / grad_xr / grad_bias next
to it against ``segger_oracle.gatv2_conv`` under float64 autograd on the same storage-rounded inputs, in all three storage
types, at the flagship geometry (H = 2, C = 64) and at (H = 3, C = 32), whose 12 lanes per row leave 4 of a 16-lane
group idle.

Tolerances: the per-dtype (atol, rtol) of tests/test_gpu_gatv2.py, scaled as there by 4 sqrt(n) with n the number of terms
the entry sums: the largest out-degree for grad_xl, the largest in-degree for grad_xr, the edge count for grad_att, the
destination count for grad_bias.
"""
import re

import pytest
import torch

from test_gpu_gatv2 import TOL, close, oracle_conv                          # noqa: F401  (TOL: the constants reused here)

GEOS = [(2, 64), (3, 32)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SEED = 0x0A77_5EED


def _features(n_src, n_dst, hc, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    xl = torch.randn(n_src, hc, generator=g).to(dtype)
    xr = torch.randn(n_dst, hc, generator=g).to(dtype)
    att = torch.randn(hc, generator=g) * 0.3
    bias = torch.randn(hc, generator=g) * 0.1
    gy = torch.randn(n_dst, hc, generator=g).to(dtype)
    return xl, xr, att, bias, gy


def _hip(cuda, graph, H, C, xl, xr, att, bias, gy, p=0.0, bits=None):
    from segger_amd import ops
    d = [t.to(cuda).requires_grad_(True) for t in (xl, xr, att, bias)]
    y = ops.gatv2_aggregate(d[0], d[1], d[2], d[3], graph, H, C, apply_gelu=True, dropout_p=p, seed=SEED, keep_bits=bits)
    y.backward(gy.to(cuda))
    torch.cuda.synchronize()
    return [t.grad for t in d]


def _check(oracle, cuda, dtype, H, C, ei, n_src, n_dst, feats=None, dropout=None, lazy=False):
    """dropout: None | "bits" | "eid" (p = 0.2).  -> the graph, for route assertions."""
    from segger_amd import ops
    from segger_amd.graph import build_edge_graph
    hc, E = H * C, int(ei.shape[1])
    xl, xr, att, bias, gy = feats if feats is not None else _features(n_src, n_dst, hc, dtype, 17 * H + C + E)
    p = 0.2 if dropout else 0.0
    keep = oracle.dropout_keep_mask(SEED, E, H, p) if dropout else None

    o = [t.double().requires_grad_(True) for t in (xl, xr, att, bias)]
    y_ref, _, _ = oracle_conv(oracle, o[0], o[1], ei, o[2], o[3], H, True, keep=keep, p=p)
    y_ref.backward(gy.double())

    graph = build_edge_graph(ei.to(cuda), n_src, n_dst, **({"need_by_src": "lazy"} if lazy else {}))
    bits = None
    if dropout == "bits":
        bits = (ops.dropout_bits(graph.by_dst, H, p, [SEED])[0],
                None if graph.by_src is None else ops.dropout_bits(graph.by_src, H, p, [SEED])[0])
    got = _hip(cuda, graph, H, C, xl, xr, att, bias, gy, p=p, bits=bits)

    deg_in = int(torch.bincount(ei[1], minlength=n_dst).max()) if E else 0
    deg_out = int(torch.bincount(ei[0], minlength=n_src).max()) if E else 0
    close(got[2], o[2].grad, dtype, scale=4.0 * max(1.0, E) ** 0.5, what="grad_att")
    close(got[0], o[0].grad, dtype, scale=4.0 * max(1.0, deg_out) ** 0.5, what="grad_xl")
    close(got[1], o[1].grad, dtype, scale=4.0 * max(1.0, deg_in) ** 0.5, what="grad_xr")
    close(got[3], o[3].grad, dtype, scale=4.0 * max(1.0, n_dst) ** 0.5, what="grad_bias")
    return graph


def _edges_with_in_degrees(deg, sources, seed):
    """COO edges: destination j gets deg[j] in-edges from random members of ``sources``, in shuffled order."""
    g = torch.Generator().manual_seed(seed)
    dst = torch.repeat_interleave(torch.arange(len(deg)), torch.as_tensor(deg))
    src = sources[torch.randint(0, len(sources), (dst.numel(),), generator=g)]
    perm = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]])


def _empty_rows_graph():
    """37 destinations with in-degrees 0..9 and 37 sources of which 30..36 have no out-edge: the last source workgroup
    holds one wave whose 4 rows are all edgeless and one whose rows lie past the end."""
    deg = [j % 10 for j in range(37)]
    return _edges_with_in_degrees(deg, torch.arange(30), seed=1), 37, 37


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
def test_empty_rows(oracle, cuda, dtype, H, C):
    ei, n_src, n_dst = _empty_rows_graph()
    out_deg = torch.bincount(ei[0], minlength=n_src)
    assert int((torch.bincount(ei[1], minlength=n_dst) == 0).sum()) == 4 and int((out_deg == 0).sum()) >= 7
    _check(oracle, cuda, dtype, H, C, ei, n_src, n_dst)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
def test_whole_source_wave_leaves_early(oracle, cuda, dtype, H, C):
    """Sources 4..7 -- the four rows of the second wave of the first source workgroup -- have no out-edge while the
    other waves of that workgroup do: the wave takes the early exit and must still hand in a zero partial."""
    n_src, n_dst = 40, 23
    sources = torch.tensor([s for s in range(n_src) if not 4 <= s < 8])
    ei = _edges_with_in_degrees([3 + j % 5 for j in range(n_dst)], sources, seed=2)
    out_deg = torch.bincount(ei[0], minlength=n_src)
    assert int(out_deg[4:8].sum()) == 0 and int(out_deg[:4].sum()) > 0 and int(out_deg[8:16].sum()) > 0
    _check(oracle, cuda, dtype, H, C, ei, n_src, n_dst)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
def test_several_workgroups_ragged_tail_and_a_long_row(oracle, cuda, dtype, H, C):
    """200 rows on either side (13 workgroups of 16 rows, the last one ragged); destination 77 has 71 in-edges: a second
    chunk of 64 neighbour ids, and a last batch that is not full."""
    n = 200
    deg = [(3 * j) % 8 for j in range(n)]
    deg[77] = 71
    ei = _edges_with_in_degrees(deg, torch.arange(n), seed=3)
    graph = _check(oracle, cuda, dtype, H, C, ei, n, n)
    assert ei.shape[1] / n < 32                                     # group-per-row on both sides


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
def test_exact_zeros_of_t(oracle, cuda, dtype, H, C):
    """x_l = -x_r on the first 8 channels of every node, so t = +-0 there on every edge: leaky_relu'(0) is taken the same
    way in both passes (the sign canonicalisation) and those channels' grad_att comes out as the oracle's."""
    ei, n_src, n_dst = _empty_rows_graph()
    hc = H * C
    xl, xr, att, bias, gy = _features(n_src, n_dst, hc, dtype, 5)
    xl[:, :8] = 0.5
    xr[:, :8] = -0.5
    xl[:, 8:12] = 0.0                                               # and 0 + (-0)
    xr[:, 8:12] = -0.0
    _check(oracle, cuda, dtype, H, C, ei, n_src, n_dst, feats=(xl, xr, att, bias, gy))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
@pytest.mark.parametrize("dropout", [None, "bits", "eid"])
def test_dropout(oracle, cuda, dtype, H, C, dropout):
    """Attention dropout 0.2 from keep-bit planes, from the hash of the edge ids, and off: a dropped edge keeps its
    logit's share of de (through D) but not its own term -- the scaling is inside de in both passes."""
    n = 90
    ei = _edges_with_in_degrees([2 + j % 9 for j in range(n)], torch.arange(n), seed=4)
    _check(oracle, cuda, dtype, H, C, ei, n, n, dropout=dropout)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
@pytest.mark.parametrize("n_src", [300, 10])
def test_wave_per_row_two_pass(oracle, cuda, dtype, H, C, n_src):
    """Destinations with 40..100 in-edges: the groups of a wave split one row in the destination pass, and -- with 10
    sources of ~84 out-edges each -- in the source pass too, where every group holds the same x_l."""
    n_dst = 12
    deg = [40 + (j * 60) // (n_dst - 1) for j in range(n_dst)]
    ei = _edges_with_in_degrees(deg, torch.arange(n_src), seed=6)
    assert ei.shape[1] / n_dst >= 32 and (ei.shape[1] / n_src >= 32) == (n_src == 10)
    graph = _check(oracle, cuda, dtype, H, C, ei, n_src, n_dst, dropout="bits")
    assert graph.by_src is not None


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
@pytest.mark.parametrize("n_src,n_dst,E", [(900, 7, 480), (500, 120, 400)])
def test_one_pass_route_with_unique_sources(oracle, cuda, dtype, H, C, n_src, n_dst, E):
    """Every source has at most one out-edge: no by-source view, no source pass, grad_att summed per edge in the
    destination pass (wave-per-row and group-per-row).  Against the oracle, at the tolerance of every other case."""
    g = torch.Generator().manual_seed(E)
    ei = torch.stack([torch.randperm(n_src, generator=g)[:E], torch.randint(0, n_dst, (E,), generator=g)])
    graph = _check(oracle, cuda, dtype, H, C, ei, n_src, n_dst, dropout="bits", lazy=True)
    assert graph.src_unique() and graph.by_src is None


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
def test_merged_small_batch_launch_equals_single_calls(cuda, dtype, H, C):
    """segger_gatv2_bwd_pair below SEGGER_BWD_PAIR_MAX_ROWS (the source pass of tx-neighbors-tx in one launch with the
    one-pass tx-belongs-bd pass) against the two single calls: the same kernel bodies built into another kernel, so -- as
    tests/test_gpu_gatv2.py states for this route -- equal to the last bit (fp32) or one rounding flip (16-bit rows), the
    parameter gradients to 1e-5 of their largest entry."""
    from segger_amd import ops
    from segger_amd.graph import build_edge_graph
    n_tx, n_bd, k, hc = 700, 9, 4, H * C
    g = torch.Generator().manual_seed(n_tx + H)
    ei_tt = torch.stack([torch.randint(0, n_tx, (n_tx * k,), generator=g), torch.arange(n_tx).repeat_interleave(k)])
    ei_tt = ei_tt[:, ei_tt[0] >= 8]                                 # sources 0..7: two edgeless source waves
    ei_tb = torch.stack([torch.randperm(n_tx, generator=g), torch.randint(0, n_bd, (n_tx,), generator=g)])
    g_tt = build_edge_graph(ei_tt.to(cuda), n_tx, n_tx)
    g_tb = build_edge_graph(ei_tb.to(cuda), n_tx, n_bd, need_by_src="lazy")
    xp_tx = torch.randn(n_tx, 3 * hc, generator=g).to(dtype)
    xp_bd = torch.randn(n_bd, hc, generator=g).to(dtype)
    vecs = [torch.randn(hc, generator=g) * s for s in (0.3, 0.1, 0.3, 0.1)]
    w_tx, w_bd = torch.randn(n_tx, hc, generator=g).to(cuda), torch.randn(n_bd, hc, generator=g).to(cuda)
    bits_tt = (ops.dropout_bits(g_tt.by_dst, H, 0.2, [11])[0], ops.dropout_bits(g_tt.by_src, H, 0.2, [11])[0])
    bits_tb = (ops.dropout_bits(g_tb.by_dst, H, 0.2, [12])[0], None)

    def leaves():
        return [t.to(cuda).requires_grad_(True) for t in [xp_tx, xp_bd] + vecs]

    def merged():
        L = leaves()
        y_tx, y_bd, _ = ops.hetero_gat_layer(*L, g_tt, g_tb, H, C, dropout_p=0.2, seed_tt=11, seed_tb=12,
                                             bits_tt=bits_tt, bits_tb=bits_tb)
        ((y_tx.float() * w_tx).sum() + (y_bd.float() * w_bd).sum()).backward()
        return [t.grad for t in L]

    def one_by_one():
        L = leaves()
        y_tx = ops.gatv2_aggregate(L[0][:, :hc], L[0][:, hc:2 * hc], L[2], L[3], g_tt, H, C, apply_gelu=True,
                                   dropout_p=0.2, seed=11, keep_bits=bits_tt)
        y_bd = ops.gatv2_aggregate(L[0][:, 2 * hc:], L[1], L[4], L[5], g_tb, H, C, apply_gelu=True, dropout_p=0.2,
                                   seed=12, keep_bits=bits_tb)
        ((y_tx.float() * w_tx).sum() + (y_bd.float() * w_bd).sum()).backward()
        return [t.grad for t in L]

    assert ops._BWD_PAIR and n_tx <= 262144 and g_tb.src_unique()
    a, b = merged(), one_by_one()
    rt = 2e-6 if dtype == torch.float32 else 2.0 ** -7
    for i, (x, y) in enumerate(zip(a[:2], b[:2])):
        assert torch.allclose(x.float(), y.float(), rtol=rt, atol=rt * float(y.float().abs().max()) * 0.25 + 1e-9), \
            f"row gradient {i}: {(x.float() - y.float()).abs().max()}"
    for i, (x, y) in enumerate(zip(a[2:], b[2:])):
        assert (x - y).abs().max() <= 1e-5 * y.abs().max() + 1e-5, f"parameter gradient {i}: {(x - y).abs().max()}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,C", GEOS)
def test_grad_att_is_deterministic(cuda, dtype, H, C):
    """Same inputs, same bits: the partials are summed in a fixed order, nothing accumulates with atomics."""
    from segger_amd.graph import build_edge_graph
    n = 200
    deg = [(3 * j) % 8 for j in range(n)]
    deg[77] = 71
    ei = _edges_with_in_degrees(deg, torch.arange(n), seed=3)
    graph = build_edge_graph(ei.to(cuda), n, n)
    feats = _features(n, n, H * C, dtype, 9)
    a = _hip(cuda, graph, H, C, *feats, p=0.2)
    b = _hip(cuda, graph, H, C, *feats, p=0.2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[2].abs().max()) > 0


def test_workspace_grows_with_the_source_count_and_abi_matches_header():
    """The two-pass workspace holds one grad_att partial per source workgroup; the one-pass size is its n_src = 0 case."""
    import os
    from segger_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segger_amd.h")).read()
    assert lib.segger_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define\s+SEGGER_ABI_VERSION\s+(\d+)", header).group(1))
    two, one = lib.segger_gatv2_bwd_workspace_bytes_two_pass, lib.segger_gatv2_bwd_workspace_bytes
    H, C = 2, 64
    sizes = [two(1000, n_src, 15 * n_src, H, C) for n_src in (0, 16, 1000, 100_000, 1_000_000)]
    assert sizes[0] == one(1000, H, C) and all(a < b for a, b in zip(sizes, sizes[1:]))
    # one [H*C] fp32 row per 16 source rows in group-per-row mode, per 4 rows once the average out-degree reaches 32
    assert sizes[-1] - sizes[0] >= 1_000_000 // 16 * H * C * 4
    assert two(1000, 1000, 32 * 1000, H, C) - sizes[0] >= 1000 // 4 * H * C * 4 > sizes[2] - sizes[0]
    assert two(0, 0, 0, H, C) == 16 and two(0, 1000, 0, H, C) > 16
