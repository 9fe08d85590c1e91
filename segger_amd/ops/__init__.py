"""Host-side operators over the C ABI: raw launch helpers + autograd Functions.

Everything here enqueues HIP kernels from ``libsegger_amd.so`` on torch's
current stream; torch is used for device memory and autograd plumbing only.
There is no CPU path (see ``_lib.require_cuda``).
"""
from __future__ import annotations

import os


# --------------------------------------------------------------------------
# Route switches
# --------------------------------------------------------------------------
# Every module-level choice between kernel routes, in one table.  The submodules read them as attributes of this package
# when they are called (``ops.FUSED_WGRAD_DX``) and never bind a copy of their own, so ``ops.NAME = value`` -- a test's
# monkeypatch, a tool's A/B flag -- reaches every route.  tools/bench_step.py sets any of them by name (NAME=0|1).

# GATv2 aggregation (gatv2.py)
# 0: always two segger_gatv2_fwd calls (A/B switch of tools/bench_step.py)
_FWD_PAIR = 1
# 0: always two segger_gatv2_bwd calls (A/B switch of tools/ab_graphed.py; tests/test_gpu_gatv2.py)
_BWD_PAIR = 1

# Loss heads (heads.py)
# packed 16-bit atomics into a gradient of the embeddings' dtype from this many triplets on: no fp32 staging + cast
# (tests/test_gpu_heads.py)
_CONTRIB_MIN_EDGES = 16384
# False = the round-3 loss head, three kernels + combination each way (tests/test_gpu_heads.py, tools/bench_loss_head.py)
ONE_LAUNCH_LOSS_HEAD = True
# The one-launch head for batches up to this many transcript rows.  Round 4 kept large batches on the kernel-by-kernel head: at
# 10^6 rows its forward (chains threaded with 4 returning atomics per triplet: 250 us against 150 us) and its gathered backward
# (-70..130 us) tied in bf16 (tools/bench_loss_head.py, profiles/r04_loss_head_modes_c2.txt).  Round 5 measured the whole C2
# step (tools/bench_step.py, alternating variants in one process): bf16 12.93-13.08 -> 12.88-12.93 ms, and at fp32 storage --
# where the kernel-by-kernel backward adds 128 M fp32 atomics -- 27.4-27.6 -> 26.5 ms: the one-launch head at every size the
# kernel's 30-bit row ids allow.
LOSS_HEAD_ONE_LAUNCH_MAX_ROWS = (1 << 30) - 2
# False = loss_tx's anchor terms by atomics at fp32 storage as well (tests/test_gpu_heads.py)
USE_ANCHOR_ROWS = True

# Projections (linear.py; the first layer in frontend.py)
# False = separate data-gradient GEMM + weight-gradient kernel (tests/test_gpu_linear.py, tools/bench_step.py FUSED_DX)
FUSED_WGRAD_DX = True
# False = the first layer's GELU derivative as an elementwise pass of its own (tests/test_gpu_model.py)
FUSED_GELU_GATE = True
# fp32 storage: forward projections and their data gradients as three-way bf16 splits on the bf16 matrix pipe
# (segger_linear_fwd_f32_split: 0.77 vs 1.17 ms for 1M x 128 -> 384) instead of the exact-fp32 MFMA.  ON by default since
# round 5: measured against fp64 its error is within the exact kernel's own (3.2e-7 vs 3.5e-7 of sum |x||w|,
# profiles/r04_f32_split.txt -- fp32 accumulation dominates both) and every fp32 parity test holds with it.  It is not
# bit-identical to a chain of fp32 FMAs: SEGGER_AMD_F32_EXACT=1 (or ops.F32_SPLIT = False) selects the exact kernels.
# (tests/test_gpu_linear.py, tools/bench_f32_wgrad.py; bench.py reports it)
F32_SPLIT = os.environ.get("SEGGER_AMD_F32_EXACT", "0") in ("", "0")
# fp32 storage: gelu' / silu' of a data gradient in the GEMM's epilogue (segger_linear_fwd_f32_gate; ist_encoder.py reads it)
F32_GATE_EPILOGUE = True
# (with F32_SPLIT) the weight gradients on the split as well (segger_linear_wgrad_f32_split)
F32_SPLIT_WGRAD = True
# False = one launch per projection
LINEAR_PAIR = True
# ... and per projection backward
WGRAD_PAIR = True

# Positional embedder (posemb.py; ist_encoder.py reads them when it names an embedder call's route, Positional2dEmbedder.route:
# where the sinusoid features come from -- "none" | "posfreq" | "torch" -- and the form of the MLP -- "fused16" | "poly_f32" |
# "mlp_f32" | "composed")
# "fused16", the whole 16-bit embedder in one kernel (ops.posmlp), where it applies; False: "posfreq" + "composed", i.e.
# linear + SiLU + linear (tests/test_gpu_model.py)
FUSED_POSMLP = True
# False = the backward of "fused16" as three kernels, round 2 (tests/test_gpu_heads.py, tools/bench_posmlp_bwd.py)
FUSED_POSMLP_BWD = True
# fp32 storage, "poly_f32": the positional embedder's first Linear as a degree-12 polynomial of the normalised coordinate
# (csrc/posenc_poly.hip) -- no [2n, 256] feature matrix (2 GB at C2: segger_posfreq wrote it, two exact-fp32 GEMMs read it)
# and no K = 256 GEMM, forward or weight gradient.  False: "posfreq" + "mlp_f32" (_MlpSiluF32, round 5's route); with
# F32_GATE_EPILOGUE off as well, or a Linear without bias: "posfreq" + "composed".
# (tests/test_gpu_model.py)
POS_POLY_F32 = True

# Encoder front end (frontend.py; ist_encoder.py reads them when it plans a step's input stage, ISTEncoder.front_plan)
# one embedder call for both node types (tests/test_host.py)
MERGED_POS_EMBED = True
# ... and one gather / concat / GELU launch for both (ops.front_join); False: per type, torch on 'bd' (tests/test_gpu_heads.py)
FRONT_JOIN = True
# large batches (one embedder call per type): both calls behind one autograd node (ops.posmlp_pair; tests/test_host.py)
POS_PAIR_NODE = True
# first-layer projections as per-gene table + positional GEMM (ops.embed_linear); its ~15 extra tiny launches (table GEMM,
# weight slices) only pay for themselves on large batches: from this many transcript rows on at 16-bit compute
# (tests/test_gpu_model.py)
SPLIT_FIRST_LAYER = True
SPLIT_FIRST_LAYER_MIN_ROWS = 200_000
# fp32 storage: the un-split first layer is a K = 256 GEMM on the exact-fp32 MFMA pipe (157 TFLOP/s) forward, backward
# and for its weight gradient -- 0.6 ms of the captured 1M-edge step's 2.4 (profiles/r06_small_batch_step_f32_*.txt) --
# while the split form's K = 128 shapes run on the bf16x3 kernels: worth it from far fewer rows
SPLIT_FIRST_LAYER_MIN_ROWS_F32 = 4_096
# False = the table and its gradients through torch ops around _RowBiasLinear (tests/test_gpu_model.py)
EMBED_LINEAR_ONE_NODE = True
# the one-node first layer for panels of up to this many genes; larger ones take the torch-composed route
EMBED_LINEAR_MAX_GENES = 1024

# --------------------------------------------------------------------------
# The operators, by subject: _common (row / vector helpers, deferred reductions, vendor-GEMM accounting), draws (random
# draws of a step), gatv2, heads (prediction head and losses), step (Adam, staging), packs (compute-dtype weight copies),
# linear (projections), posemb (positional embedder), frontend (encoder input / tail).
# --------------------------------------------------------------------------
from .. import _lib                    # (bench.py reads ops._lib)
from ._common import _vendor_gemm, deferred_reductions, vendor_gemm_calls
from .draws import dropout_bits, dropout_bits_many, sample_negatives, step_advance, step_draws, triplet_sample
from .gatv2 import (gatv2_aggregate, gatv2_bwd_launch, gatv2_bwd_pair_launch, gatv2_fwd_launch, gatv2_fwd_pair_launch,
                    hetero_gat_layer)
from .heads import (LossHeadSpec, _LossHead, _TICKETS, _triplet_args, anchor_index, bce_edge_loss, edge_cos_argmax,
                    loss_head, loss_head_fused_supported, loss_head_route, metric_loss, triplet_edge_loss)
from .step import (GradWindow, GuardState, accumulate_batches, adam_hyper, adam_init_state, adam_step, adam_step_counters,
                   double_bits, float_bits, grad_accumulate, grad_guard, stage, window_flush)
from .packs import (_PACKS, _pack_for, alias_of, f32_split_planes, invalidate_weight_cache, invalidate_weights, pack_scope,
                    packs_of)
from .linear import (colsum, linear, linear_f32_act_launch, linear_f32_gate_launch, linear_f32_gate_supported,
                     linear_f32_split_launch, linear_f32_split_supported, linear_fwd_launch, linear_fwd_pair_launch,
                     linear_pair, linear_supported, linear_wgrad_dx_gate_supported, linear_wgrad_dx_launch,
                     linear_wgrad_dx_supported, linear_wgrad_launch, linear_wgrad_pair_launch, linear_wgrad_supported,
                     segment_rowsum)
from .posemb import (mlp_silu_f32, mlp_silu_f32_covers, mlp_silu_f32_supported, pos_poly_f32_covers, pos_poly_mlp_f32,
                     pos_poly_mlp_f32_supported, posfreq, posmlp, posmlp_pair, posmlp_pair_supported, posmlp_supported,
                     segment_minmax)
from .frontend import (EmbedInput, _EmbedLinear, _gene_table_args, embed_gelu, embed_linear, embed_linear_supported,
                       front_join, l2_normalize, l2_normalize_many, rows_by_id)
