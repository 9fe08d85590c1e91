/*
 * segger_amd.h -- C ABI of libsegger_amd.so: hand-written gfx950 (MI355X) HIP
 * kernels for segger's GNN hot path (heterogeneous GATv2 message passing over
 * transcript<->boundary graphs + the transcript->cell edge-scoring heads).
 *
 * The reference (dpeerlab/segger) has no FFI for this path: the arithmetic is
 * reached through Python calls into torch_geometric / torch_scatter / torch
 * CUDA kernels.  Each entry point below names the reference call site (file:line
 * under /root/reference) whose third-party kernel(s) it replaces.
 *
 * Conventions (every entry point):
 *   - returns SEGGER_OK (0) or a negative SEGGER_E* code; segger_last_error()
 *     returns a thread-local message for the last failure on this thread;
 *   - never throws, never allocates or frees device memory, never synchronises:
 *     work is only enqueued on `stream` (a hipStream_t; NULL = default stream);
 *   - all pointers are DEVICE pointers borrowed for the duration of the enqueued
 *     work; outputs and workspaces are caller-allocated
 *     (sizes from the matching *_workspace_bytes());
 *   - sizes / offsets / leading dimensions are int64_t (cf. the >2^31 element
 *     hazard in reference src/segger/_patches.py:1-9); node ids inside CSR
 *     arrays are int32_t, so one batch holds < 2^31 nodes and < 2^31 edges
 *     per edge type;
 *   - "ld_*" = row stride in ELEMENTS of the tensor's dtype; rows must be
 *     16-byte aligned (ld * sizeof(elem) % 16 == 0 and base % 16 == 0);
 *   - feature tensors are row-major [n, heads*channels] in `dtype`
 *     (SEGGER_F32 / SEGGER_BF16 / SEGGER_F16); all accumulation is fp32;
 *     parameters (att, bias) and their gradients are fp32.
 */
#ifndef SEGGER_AMD_H
#define SEGGER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: only what is declared between this push and the pop at the end of the
 * header -- the C entry points -- reaches its dynamic symbol table (a definition takes the visibility of its first
 * declaration); the C++ launchers behind them (namespace segger) stay internal. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SEGGER_ABI_VERSION 32

enum segger_status {
  SEGGER_OK = 0,
  SEGGER_EINVAL = -1,       /* bad argument (null pointer, negative size, misaligned ld) */
  SEGGER_EUNSUPPORTED = -2, /* valid but not implemented (heads/channels combination, dtype) */
  SEGGER_EHIP = -3,         /* a HIP runtime call failed; message has hipGetErrorString */
  SEGGER_EWORKSPACE = -4    /* workspace too small */
};

enum segger_dtype { SEGGER_F32 = 0, SEGGER_BF16 = 1, SEGGER_F16 = 2 };

typedef void* segger_stream_t; /* hipStream_t */

int segger_abi_version(void);
const char* segger_last_error(void);

/* ------------------------------------------------------------------------
 * Compressed sparse rows of one edge type.
 *   rows = the node the kernel iterates over, col = the node it gathers.
 *   eid[slot] = position of that edge in the caller's COO edge_index, used
 *   (a) for outputs indexed by original edge id, (b) as the dropout counter so
 *   forward, dst-side backward and src-side backward draw the same mask.
 * ---------------------------------------------------------------------- */
typedef struct segger_csr {
  const int64_t* indptr; /* [n_rows + 1] */
  const int32_t* col;    /* [n_edges] */
  const int32_t* eid;    /* [n_edges] */
  int64_t n_rows;
  int64_t n_cols;
  int64_t n_edges;
  const int32_t* row_order; /* [n_rows] or NULL: the order in which kernels visit the rows (a permutation of
                               0..n_rows-1 from segger_csr_row_order); results never depend on it */
  /* optional block tables (segger_csr_block_tables; all three or none): per workgroup of SEGGER_BLOCK_ROWS consecutive
   * visiting positions the DISTINCT column ids its rows gather -- staged in LDS once, then gathered from there */
  const int32_t* blk_cnt;   /* [ceil(n_rows / SEGGER_BLOCK_ROWS)]: number of distinct ids, <= SEGGER_BLOCK_CAP */
  const int32_t* blk_src;   /* [n_blocks][SEGGER_BLOCK_CAP]: the ids (slot order arbitrary) */
  const uint8_t* col_local; /* [n_edges]: per CSR slot, the LDS slot of col[slot] in its block's table */
} segger_csr;
#define SEGGER_BLOCK_ROWS 16
#define SEGGER_BLOCK_CAP 128
/*
 * segger_csr_block_tables: the block tables of a CSR view in a given visiting order (row_order NULL: natural).  A kNN graph
 * over spatially sorted nodes re-uses its gathered rows heavily inside a workgroup (C2 tile: the 16 rows of a workgroup
 * gather 240 rows of which 58 are distinct), so the aggregation kernels can load each distinct row ONCE per workgroup,
 * coalesced, into LDS and gather from there instead of issuing 240 row gathers through the texture addresser.
 * *overflow (device int32, zeroed by the caller) is set when some block has more than SEGGER_BLOCK_CAP distinct ids or more
 * than 1024 edges: the tables are then unusable and the caller keeps the plain kernels.
 */
int segger_csr_block_tables(const int64_t* indptr, const int32_t* col, const int32_t* row_order, int64_t n_rows, int64_t n_edges,
                            int32_t* blk_cnt, int32_t* blk_src, uint8_t* col_local, int32_t* overflow, segger_stream_t stream);

/*
 * segger_csr_from_coo: stable sort of COO edges by `row`, producing indptr /
 * col / eid.  Replaces what PyG does implicitly per layer with scatter
 * kernels keyed on edge_index[1] (GATv2Conv.propagate; constructed at
 * src/segger/models/ist_encoder.py:111-124) and torch_scatter.scatter_max's
 * keying on edge_index[0] (src/segger/models/lightning_model.py:280-284):
 * built ONCE per batch and shared by all layers, forward and backward.
 *   row, colv : [n_edges] int64 (edge_index rows as PyG stores them)
 *   n_invalid : optional device int32; receives the number of edges whose row
 *               or col id is out of range (such ids are clamped to 0 so later
 *               kernels cannot fault; the host wrapper raises on n_invalid>0).
 */
size_t segger_csr_from_coo_workspace_bytes(int64_t n_edges, int64_t n_rows);
int segger_csr_from_coo(const int64_t* row, const int64_t* colv, int64_t n_edges,
                        int64_t n_rows, int64_t n_cols,
                        int64_t* indptr, int32_t* col, int32_t* eid,
                        int32_t* n_invalid,
                        void* workspace, size_t workspace_bytes,
                        segger_stream_t stream);

/*
 * segger_csr_row_order: a visiting order for the rows of a CSR that balances the lanes of a wavefront.
 * The aggregation kernels give each 16-lane group of a wave its own row; a wave is busy until its
 * longest row is done, so rows of unequal degree (kNN in-degrees: mean k, spread ~ sqrt(k)) idle lanes.
 * Inside every window of `window` consecutive rows (a power of two <= 64, so neighbouring rows still
 * share an L2) the rows are ordered by descending degree: the 4 rows of a wave then have near-equal
 * length.  order_out[n_rows] is a permutation of 0..n_rows-1.
 */
int segger_csr_row_order(const int64_t* indptr, int64_t n_rows, int32_t window,
                         int32_t* order_out, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * GATv2 attention aggregation (the roofline kernel).
 *
 * Replaces torch_geometric.nn.GATv2Conv.edge_update + utils.softmax + message
 * + aggregate('add') + bias (PyG 2.7.0), i.e. everything in the conv AFTER
 * lin_l / lin_r, for one edge type of segger's HeteroConv
 * (src/segger/models/ist_encoder.py:109-134,183-189), with the following GELU
 * (ist_encoder.py:325) optionally fused:
 *
 *   e[i->j,h]  = sum_c att[h,c] * leaky_relu(x_l[i,h,c] + x_r[j,h,c], slope)
 *   a[i->j,h]  = softmax over the in-edges of j ;  a *= keep/(1-p) (dropout)
 *   pre[j,h,c] = sum_i a[i->j,h] * x_l[i,h,c] + bias[h,c]
 *   out        = apply_gelu ? gelu_erf(pre) : pre
 *                (exact-erf GELU, torch approximate='none'; evaluated through a polynomial erfc with
 *                |error| <= 4e-7 in fp32, see csrc/common.h::normal_cdf)
 *
 * A destination without in-edges gets pre = bias.
 * Dropout (ist_encoder.py:116,123; training only), with (lo, hi) = halves of splitmix64(seed + *seed_dev):
 *   x = (eid*H + h) ^ lo;  x *= 0x85ebca6b; x ^= x>>13; x *= 0xc2b2ae35; x ^= x>>16; x ^= hi;
 *   keep(e,h) = (x >> 8) >= floor(p * 2^24)      (uint32 arithmetic).
 * ---------------------------------------------------------------------- */
typedef struct segger_gatv2_fwd_args {
  segger_csr by_dst;      /* rows = destination nodes, col = source ids */
  const void* x_l;        /* [n_src, H*C] lin_l(x_src) */
  int64_t ld_xl;
  const void* x_r;        /* [n_dst, H*C] lin_r(x_dst) */
  int64_t ld_xr;
  const float* att;       /* [H*C] */
  const float* bias;      /* [H*C] or NULL */
  int32_t heads;
  int32_t channels;
  int32_t dtype;          /* segger_dtype of x_l, x_r, out, pre */
  int32_t apply_gelu;
  float negative_slope;   /* 0.2 in GATv2Conv */
  float dropout_p;        /* 0 = eval */
  uint64_t seed;
  const uint64_t* seed_dev; /* optional DEVICE word: the effective seed is seed + *seed_dev, read when the kernel
                               runs (a captured hipGraph draws a fresh mask every replay); NULL = seed alone */
  void* out;              /* [n_dst, H*C] */
  int64_t ld_out;
  void* pre;              /* [n_dst, H*C] pre-activation for backward; NULL = skip
                             (may alias out when !apply_gelu) */
  int64_t ld_pre;
  float* lse;             /* [n_dst, H] log2(sum exp2(e*log2(e))) per (dst, head), kernel units;
                             NULL = skip */
  float* alpha;           /* [n_edges, H] attention (after dropout) by ORIGINAL edge id; NULL = skip
                             (SkipGAT.attention_weights, ist_encoder.py:146-158,192-211) */
  const uint8_t* keep_bits; /* optional, [n_edges] in by_dst SLOT order: bit h = keep(e, h) of the mask defined
                               above, precomputed by segger_dropout_bits for this layer's seed.  The kernels then test
                               a bit instead of hashing per (edge, head); results are identical.  Ignored when alpha
                               is requested or the geometry runs on the generic kernels. */
} segger_gatv2_fwd_args;

int segger_gatv2_fwd(const segger_gatv2_fwd_args* args, segger_stream_t stream);
/* Two edge types of one HeteroConv layer (ist_encoder.py:109-134: tx-neighbors-tx and tx-belongs-bd) in ONE launch: the
 * few thousand short blocks of the high-degree edge type `b` (wave per destination row) run beside the blocks of the
 * low-degree edge type `a` (lane group per row) instead of as a latency-bound launch of their own.  Same arguments as
 * two segger_gatv2_fwd calls; falls back to two launches when the pair is not (group-per-row, wave-per-row) of one
 * specialised geometry and storage type, or when attention weights are requested. */
int segger_gatv2_fwd_pair(const segger_gatv2_fwd_args* a, const segger_gatv2_fwd_args* b, segger_stream_t stream);

/*
 * Backward of the above (replaces autograd through the PyG ops).  Two atomic-free
 * passes: a destination-side pass (CSR by dst) producing grad_pre, grad_xr,
 * grad_att, grad_bias, and a source-side pass (CSR by src) producing grad_xl.
 * Attention coefficients are recomputed from x_l, x_r and `lse`; no [E,H,C]
 * tensor is ever materialised.  Outputs are WRITTEN (not accumulated).
 */
typedef struct segger_gatv2_bwd_args {
  segger_csr by_dst;      /* as in forward */
  segger_csr by_src;      /* rows = source nodes, col = destination ids (same edges) */
  const void* x_l;
  int64_t ld_xl;
  const void* x_r;
  int64_t ld_xr;
  const float* att;
  const float* bias;      /* may be NULL */
  int32_t heads;
  int32_t channels;
  int32_t dtype;
  int32_t apply_gelu;
  float negative_slope;
  float dropout_p;
  uint64_t seed;
  const uint64_t* seed_dev; /* as in forward; must hold the value the forward saw */
  const void* grad_out;   /* [n_dst, H*C] dL/d out */
  int64_t ld_go;
  const void* pre;        /* [n_dst, H*C] from forward */
  int64_t ld_pre;
  const float* lse;       /* [n_dst, H] from forward */
  void* grad_pre;         /* [n_dst, H*C] scratch+output: dL/d pre (dtype) */
  int64_t ld_gp;
  float* dsum;            /* [n_dst, H, 2] scratch: (lse, D) pairs, D = sum_c grad_pre * (pre - bias) */
  void* grad_xl;          /* [n_src, H*C] */
  int64_t ld_gxl;
  void* grad_xr;          /* [n_dst, H*C] */
  int64_t ld_gxr;
  float* grad_att;        /* [H*C] */
  float* grad_bias;       /* [H*C] or NULL */
  void* workspace;        /* segger_gatv2_bwd_workspace_bytes_two_pass(); with src_unique set
                             segger_gatv2_bwd_workspace_bytes() suffices */
  size_t workspace_bytes;
  const uint8_t* keep_bits_dst; /* optional dropout bit planes (see forward) in by_dst / by_src slot order */
  const uint8_t* keep_bits_src;
  int32_t src_unique;     /* non-zero: the caller asserts that no source node has more than one out-edge (segger's
                             tx-belongs-bd: a transcript lies in at most one boundary; check with
                             segger_coo_unique).  grad_xl[i] then has a single term, the destination-side pass
                             stores it itself and by_src is ignored (may be all zero): no by-source sort, no
                             source-side pass.  Needs a specialised geometry (segger_gatv2_has_specialised). */
  void* zero_rows_out;    /* optional, two-pass form only: a second [n_src, H*C] matrix (row stride ld_zero) that the
                             source pass zero-fills row by row while it writes grad_xl -- the grad_xl of ANOTHER edge
                             type over the same source nodes whose one-pass backward runs next (segger: tx-neighbors-tx
                             fills the tx-belongs-bd window of the stacked projection gradient) */
  int64_t ld_zero;
  int32_t grad_xl_zeroed; /* one-pass form (src_unique): grad_xl already holds zeros (see zero_rows_out): skip the fill */
  int32_t passes;         /* segger_gatv2_bwd only -- 0: the whole backward (default); 1: the destination-side pass alone
                             (grad_pre, dsum, grad_xr, grad_bias; grad_xl and grad_att too in the one-pass form); 2: the
                             source-side KERNEL alone (grad_xl from the grad_pre / dsum an earlier passes = 1 call left in
                             the same buffers; grad_att / grad_bias are not written).  Exists so that a profiler / bench.py
                             can time the two kernels of the backward separately (roofline.dominant): 1 then 2 gives the
                             row gradients and grad_bias of 0.  grad_att of the two-pass form is a sum over both passes'
                             rows (per destination x_r * (c1 Sde + c2 Sg), per source x_l * (c1 Sde + c2 Sg), with Sde /
                             Sg the row's sums of de and de * sgn(t)): only passes = 0 sums both halves; passes = 1 leaves
                             the destination half alone in grad_att.  3: the destination KERNEL alone -- as 1 without
                             the two small launches that sum its per-workgroup grad_att / grad_bias partials (those two
                             outputs are then not written): timing only. */
} segger_gatv2_bwd_args;

/* Workspace of the one-pass form (src_unique) -- equal to the two-pass size for n_src = 0. */
size_t segger_gatv2_bwd_workspace_bytes(int64_t n_dst, int32_t heads, int32_t channels);
/* Workspace of the two-pass form: the destination pass's per-workgroup partials of grad_att / grad_bias, the source
 * pass's per-workgroup partials of grad_att (one [H*C] row per workgroup of by-source rows: grows with n_src; n_edges
 * decides between 4 and 4 * (64 / group size) source rows per workgroup as the launcher does) and the partials of their
 * deterministic sum.  Purely additive: one new symbol, no existing signature or struct changes, so SEGGER_ABI_VERSION
 * stays 32; a two-pass call handed only segger_gatv2_bwd_workspace_bytes() returns SEGGER_EWORKSPACE. */
size_t segger_gatv2_bwd_workspace_bytes_two_pass(int64_t n_dst, int64_t n_src, int64_t n_edges, int32_t heads,
                                                 int32_t channels);
int segger_gatv2_bwd(const segger_gatv2_bwd_args* args, segger_stream_t stream);
/* The backward of both edge types of one HeteroConv layer (ist_encoder.py:109-134 under autograd): `a` a two-pass edge
 * type (tx-neighbors-tx), `b` a one-pass one (src_unique: tx-belongs-bd) whose grad_xl is the matrix `a` zero-fills
 * (a->zero_rows_out == b->grad_xl with b->grad_xl_zeroed set, or neither set).  Same results as segger_gatv2_bwd(a)
 * followed by segger_gatv2_bwd(b) (b's row gradients and sums to rounding: inside the merged kernel its body walks
 * another number of rows at a time and sums grad_att by endpoint).  At every batch size -- unless the environment
 * variable SEGGER_BWD_PAIR_MAX_ROWS (read once) caps the source nodes of `a` up to which this happens; 0: never -- for
 * one specialised geometry and storage type, with `b` in wave-per-row mode and a's destinations and b's sources
 * indexing the same nodes, the zero fill moves into a's DESTINATION pass, a's source pass shares ONE launch with b's
 * destination pass (b's latency-bound blocks run beside a's), and the slab sums of both edge types share one launch
 * pair; otherwise the two calls run as they are.  SEGGER_BWD_ONE_PASS_IN_PAIR_KERNEL=1 (read once) makes
 * segger_gatv2_bwd launch a wave-per-row one-pass backward as that merged kernel with an empty `a` side: the merged
 * launch's body for `b` by itself, bit for bit, for comparisons and timing. */
int segger_gatv2_bwd_pair(const segger_gatv2_bwd_args* a, const segger_gatv2_bwd_args* b, segger_stream_t stream);
/*
 * segger_dropout_bits: the attention-dropout mask of n_seeds layers as bit planes over the slots of one CSR view:
 *   bits[l * plane_stride + slot] = sum_h keep(eid[slot], h; seeds[l] + *seed_dev) << h        (heads <= 8)
 * with keep() exactly the counter-based mask of segger_gatv2_fwd.  One launch per view per training step replaces
 * 3 passes x n_seeds layers of per-(edge, head) hashing inside the aggregation kernels.  seeds is a HOST array.
 * plane_stride: bytes between the planes of consecutive layers, a multiple of 4 and >= n_edges (a thread writes four
 * slots of a plane as one word); bits 4-byte aligned.
 */
int segger_dropout_bits(const int32_t* eid, int64_t n_edges, int32_t heads, float dropout_p, const uint64_t* seeds,
                        int32_t n_seeds, const uint64_t* seed_dev, uint8_t* bits, int64_t plane_stride,
                        segger_stream_t stream);
/* segger_dropout_bits_many: up to 4 such views (the by-destination / by-source views of a step's edge types) in ONE
 * launch; per view the arguments of segger_dropout_bits.
 * segger_step_advance: *step += inc and (optionally) *copy = the new value, one tiny launch -- the device-side step
 * counter behind seed_dev (ISTEncoder's dropout stream), advanced and snapshotted for the backward. */
typedef struct segger_bits_job {
  const int32_t* eid;
  int64_t n_edges;
  const uint64_t* seeds;    /* HOST array [n_seeds] */
  int32_t n_seeds;
  int32_t reserved_;
  uint8_t* bits;
  int64_t plane_stride;
} segger_bits_job;
int segger_dropout_bits_many(const segger_bits_job* jobs, int32_t n_jobs, int32_t heads, float dropout_p,
                             const uint64_t* seed_dev, segger_stream_t stream);
int segger_step_advance(int64_t* step, int64_t inc, int64_t* copy, segger_stream_t stream);

/* segger_step_draws: ALL random draws of one training step in one launch -- the bit planes of up to four edge views
 * (segger_dropout_bits_many), up to two cluster-aware triplet samplers (segger_triplet_sample: loss_tx and loss_bd,
 * models/triplet_loss.py:83-125, with the kernel's own counter-based uniforms) and the negative boundaries of the
 * segmentation loss (segger_sample_negatives, lightning_model.py:167-176).  Same streams, same results as the separate
 * calls with the same seeds; every job reads the device word seed_dev. */
typedef struct segger_sample_job {
  const int64_t* lab; int64_t n; int32_t n_clusters; int32_t reserved_;
  const float* cdf_pos; const float* cdf_neg; const int64_t* counts; const int64_t* offsets; const int64_t* members;
  uint64_t seed; const float* dists; int64_t* pos; int64_t* neg; float* d_pos; float* d_neg;
} segger_sample_job;
typedef struct segger_step_draws_args {
  const segger_bits_job* bits; int32_t n_bits; int32_t heads; float dropout_p; int32_t n_samplers;
  segger_sample_job samplers[2];
  const int64_t* neg_pos; int64_t neg_n; int64_t neg_n_b; const int64_t* neg_n_b_dev; uint64_t neg_seed; int64_t* neg_out;
  const uint64_t* seed_dev;
  float* const* advance; int32_t n_advance; int32_t reserved_;   /* HOST array of up to 64 device floats: *advance[i] += 1 (Adam's
                                                                    step counters, see segger_adam_step_ex) */
} segger_step_draws_args;
int segger_step_draws(const segger_step_draws_args* args, segger_stream_t stream);

/* 1 when (heads, channels) runs on the specialised kernels (channels in {32,64}, heads in 1..4), 0 = generic kernels */
int segger_gatv2_has_specialised(int32_t heads, int32_t channels);

/*
 * segger_coo_unique: *unique_out = 1 when no value occurs twice in ids[n] (values in [0, n_ids)), else 0.
 * marks: caller-provided int32[n_ids] scratch (zeroed by the call).  Enqueue-only; read unique_out after the stream
 * has passed.  Used once per batch on edge_index[0] of tx-belongs-bd (src/segger/data/utils/heterodata.py:147: each
 * transcript is assigned to at most one boundary) to license src_unique above.
 */
int segger_coo_unique(const int64_t* ids, int64_t n, int64_t n_ids, int32_t* marks, int32_t* unique_out,
                      segger_stream_t stream);

/*
 * segger_stage: n_segs independent "copy a prefix, fill the rest" jobs in one launch -- how a batch is written into the
 * static, padded buffers a captured training step (hipGraph) replays on (no counterpart in the reference, which
 * re-launches every op of every step; lightning_model.py:151-231 is what the captured step computes).
 * Element i of segment s:   i < n_copy: src[i] (read as src_bytes-wide integer, stored dst_bytes-wide; equal sizes
 * copy bit patterns, so floats pass unchanged);  otherwise with k = i - n_copy:
 *   SEGGER_FILL_CONST  a                       (bit pattern of the value, e.g. 0 for 0.0f)
 *   SEGGER_FILL_TILE   src[k % a]              (replicate the first a elements: "copies of row 0")
 *   SEGGER_FILL_DIV    a + k / b               (b = 1: an iota)
 *   SEGGER_FILL_MOD    a + k % b
 *   SEGGER_FILL_RAMP   a + min((k + 1) * b, c) (row pointers of rows holding b padding edges each, c in total)
 * segs is a HOST array (copied into the kernel arguments).
 */
enum { SEGGER_FILL_CONST = 0, SEGGER_FILL_TILE = 1, SEGGER_FILL_DIV = 2, SEGGER_FILL_MOD = 3, SEGGER_FILL_RAMP = 4 };
typedef struct {
  void* dst;
  const void* src;
  int64_t n_copy, n_total;   /* elements */
  int64_t a, b, c;           /* fill parameters */
  int32_t dst_bytes, src_bytes;
  int32_t fill;
  int32_t copy_add;          /* added to every copied and TILE-replicated element (INTEGER segments only), e.g. to
                                rebase ids while they are copied; 0 for float segments */
} segger_stage_seg;
int segger_stage(const segger_stage_seg* segs, int32_t n_segs, segger_stream_t stream);

/*
 * segger_adam_step: torch.optim.Adam.step() (lightning_model.py:300-303: Adam(lr), default betas / eps, no weight decay,
 * no amsgrad) for n_tensors fp32 parameter tensors at once, on the optimizer's OWN state tensors (exp_avg, exp_avg_sq and
 * the per-tensor fp32 step counter of a capturable torch Adam), so checkpoints and an eager optimizer.step() stay
 * interchangeable:   step += 1;  exp_avg = lerp(exp_avg, grad, 1 - beta1);  exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) grad^2;
 * param -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps).
 * Two launches per 64 tensors (counters, then all elements) instead of torch's three multi-tensor launches per step.
 * lr / betas / eps are doubles as torch holds them (1 - beta and beta^step are evaluated in double, the rest in fp32).
 * tensors is a HOST array (copied into the kernel arguments); zero-sized tensors only advance their counter.
 */
typedef struct segger_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;               /* device scalar, fp32 (torch's capturable step counter) */
  int64_t numel;
} segger_adam_tensor;
int segger_adam_step(const segger_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2, double eps,
                     segger_stream_t stream);
/* segger_adam_step_ex: the same with (a) flags & SEGGER_ADAM_STEPS_ADVANCED: the step counters have been advanced already
 * (segger_step_draws does it at the head of a captured training step: nothing in between reads them) -- one launch instead
 * of two; (b) counter != NULL: *counter += counter_inc by the update launch's first workgroup -- the device-side dropout /
 * sampling counter of the step that ends here (nothing reads it after the backward). */
#define SEGGER_ADAM_STEPS_ADVANCED 1
int segger_adam_step_ex(const segger_adam_tensor* tensors, int32_t n_tensors, double lr, double beta1, double beta2, double eps,
                        int32_t flags, int64_t* counter, int64_t counter_inc, segger_stream_t stream);
/* segger_adam_step_dev: segger_adam_step_ex with {lr, beta1, beta2, eps} read from a DEVICE array of four doubles when the
 * kernel runs (not validated: the caller writes what its optimizer's param_group holds).  A captured training step keeps the
 * array in its static buffers and refreshes it with the batch (segger_stage), so a learning-rate scheduler that changes
 * `param_groups[0]["lr"]` every step (lightning_model.py:300-303 returns a bare Adam; schedulers are the user's) is followed
 * by the replayed graph without a new capture. */
int segger_adam_step_dev(const segger_adam_tensor* tensors, int32_t n_tensors, const double* hyper, int32_t flags,
                         int64_t* counter, int64_t counter_inc, segger_stream_t stream);

/*
 * The gradient guard: what stands between loss.backward() and optimizer.step() in a mixed-precision training loop --
 *   scaler.unscale_(opt); torch.nn.utils.clip_grad_norm_(params, max_norm); scaler.step(opt); scaler.update()
 * (torch/nn/utils/clip_grad.py, torch/amp/grad_scaler.py) -- decided ON THE DEVICE, without a host synchronisation, so
 * that a captured training step (hipGraph) can carry it.  The reference leaves all three to Lightning
 * (`gradient_clip_val`, the precision plugin); a replayed graph is out of Lightning's reach.
 *
 * segger_guard_state (DEVICE, 40 bytes, 8-byte aligned; the caller initialises scale > 0 and zeroes the rest):
 *   coef            what segger_adam_step_guarded multiplies every gradient by: clip / scale   (0 on a skipped step)
 *   skip            1: some gradient element is inf or NaN -- GradScaler's found_inf; the update writes nothing
 *   norm            the global L2 norm of the UNSCALED gradients, sqrt(sum g^2) / scale (clip_grad_norm_'s return value);
 *                   NaN on a skipped step
 *   scale           the loss scale the NEXT backward is seeded with (GradScaler._scale)
 *   growth_tracker  clean steps since the scale last changed (GradScaler._growth_tracker)
 *   n_skipped, n_clipped   running totals (steps skipped; steps with clip < 1)
 * All arithmetic in double until the last cast, with `scale` the value the state held when the call began:
 *   true_norm = sqrt(sum) / scale;   clip = max_norm > 0 ? min(1, max_norm / (true_norm + 1e-6)) : 1   (torch's formula)
 *   coef = (float)(clip / scale);    skip = any non-finite element
 *   growth_interval > 0 (a dynamic scale), as GradScaler.update:  skip: scale *= backoff, tracker = 0;  otherwise
 *   tracker += 1 and, when it reaches growth_interval, scale *= growth, tracker = 0.   growth_interval == 0: a static scale.
 *
 * segger_grad_guard: two passes over the table segger_adam_step takes (only grad, step and numel are read), in the
 * update's own (tensor, offset) blocks of 2048 elements, 64 tensors a launch.  Pass 1, one workgroup per block: the block's
 * sum of grad^2 in float64 and its any-non-finite bit into the block's workspace slot; pass 2, ONE workgroup: the slots
 * summed first to last, the state written.  Every sum has one fixed order and nothing is added atomically: the same
 * gradients give the same bytes on every run.  On a skipped step with cfg.flags & SEGGER_ADAM_STEPS_ADVANCED pass 2 takes
 * 1.0f off every step counter of the table again (torch's fused Adam: _foreach_sub_(steps, found_inf)).
 * cfg is a HOST struct (copied into the kernel arguments); n_tensors == 0 does nothing.  Enqueue-only.
 * workspace: segger_grad_guard_workspace_bytes(n_tensors, total_blocks) bytes, 256-byte aligned, total_blocks = the sum
 * over the tensors of ceil(numel / 2048): 16 bytes a block + 8 bytes a tensor, each region rounded up to 256.
 *
 * segger_adam_step_guarded: segger_adam_step_dev with g * state->coef for g (one fp32 multiply) and, when state->skip is
 * set, no tensor byte written; *counter still advances.  Without SEGGER_ADAM_STEPS_ADVANCED its counter launch adds 1
 * only when skip == 0.
 */
typedef struct segger_guard_state {
  float coef;
  int32_t skip;
  double norm;
  float scale;
  int32_t growth_tracker;
  int64_t n_skipped;
  int64_t n_clipped;
} segger_guard_state;
typedef struct segger_guard_cfg {
  double max_norm;           /* 0: no clipping */
  double growth;             /* >= 1 */
  double backoff;            /* in (0, 1) */
  int32_t growth_interval;   /* 0: static scale */
  int32_t flags;             /* SEGGER_ADAM_STEPS_ADVANCED */
} segger_guard_cfg;
int64_t segger_grad_guard_workspace_bytes(int32_t n_tensors, int64_t total_blocks);
int segger_grad_guard(const segger_adam_tensor* tensors, int32_t n_tensors, const segger_guard_cfg* cfg,
                      segger_guard_state* state, void* workspace, int64_t workspace_bytes, segger_stream_t stream);
int segger_adam_step_guarded(const segger_adam_tensor* tensors, int32_t n_tensors, const double* hyper, int32_t flags,
                             int64_t* counter, int64_t counter_inc, const segger_guard_state* state, segger_stream_t stream);

/*
 * Gradient accumulation over a window of N micro-steps (Lightning's accumulate_grad_batches) for a captured training step:
 * every replay runs backward, segger_grad_accumulate, [segger_grad_guard_windowed,] segger_adam_step_windowed, and the
 * DEVICE decides which of them act -- one graph serves every position of the window, the host decides nothing per step.
 *
 * segger_accum_window (DEVICE, 16 bytes, 4-byte aligned; the caller zeroes it once):
 *   pos      micro-steps summed into the open window (0: none -- the next accumulate OVERWRITES the accumulators)
 *   close    1: the last segger_grad_accumulate (or a flush) closed the window; what the windowed guard / update act on
 *   arrived  the accumulate launch's workgroup ticket (0 between launches)
 *
 * segger_grad_accumulate: acc = pos == 0 ? g * w : acc + g * w for all tensors in one launch per 64, w = (float)1 / n_window;
 * the table is segger_adam_step's with `grad` = the micro-step's gradient (read) and `param` = the fp32 ACCUMULATOR
 * (written; the other fields are not read).  Then pos += 1, close = (pos == n_window), and a closed window's pos is 0.
 * One thread owns an element; multiply and add are rounded separately; the sum of an element is formed in micro-step
 * order; no float atomics: the same gradients give the same bytes.  Enqueue-only.
 * segger_grad_guard_windowed / segger_adam_step_windowed: segger_grad_guard / segger_adam_step_guarded on a table whose
 * `grad` is the accumulator, acting only when window->close is set: otherwise the guard's state, the step counters, the
 * moments and the parameters keep their bytes (*counter still advances: every micro-batch draws fresh numbers).  `state`
 * of the update may be NULL (no guard).  SEGGER_ADAM_STEPS_ADVANCED is refused: the counters move in the update's own
 * counter launch, when the window closes and the step is not skipped.
 * segger_accum_window_flush: phase 0: close = (pos > 0) -- what follows applies the sum so far, every term still weighted
 * 1 / n_window; phase 1: pos = close = 0.  (Lightning closes an open window at the end of an epoch.)
 * csrc/grad_accum.hip (templates shared with adam.hip: csrc/adam_common.h).  Purely additive: four new symbols, no existing signature or struct changes, SEGGER_ABI_VERSION stays 32.
 */
typedef struct segger_accum_window {
  int32_t pos;
  int32_t close;
  int32_t arrived;
  int32_t reserved_;
} segger_accum_window;
int segger_grad_accumulate(const segger_adam_tensor* tensors, int32_t n_tensors, int32_t n_window, segger_accum_window* window,
                           segger_stream_t stream);
int segger_grad_guard_windowed(const segger_adam_tensor* tensors, int32_t n_tensors, const segger_guard_cfg* cfg,
                               segger_guard_state* state, void* workspace, int64_t workspace_bytes,
                               const segger_accum_window* window, segger_stream_t stream);
int segger_adam_step_windowed(const segger_adam_tensor* tensors, int32_t n_tensors, const double* hyper, int32_t flags,
                              int64_t* counter, int64_t counter_inc, const segger_guard_state* state,
                              const segger_accum_window* window, segger_stream_t stream);
int segger_accum_window_flush(segger_accum_window* window, int32_t phase, segger_stream_t stream);

/* segger_transpose_many: dst [cols, rows] = src [rows, cols]^T for n_segs contiguous 16-bit matrices in one launch:
 * the W^T copies the data-gradient GEMMs (dX = dY W on segger_linear_fwd) need after every optimizer step. */
typedef struct {
  void* dst;
  const void* src;
  int32_t rows, cols;
} segger_transpose_seg;
int segger_transpose_many(const segger_transpose_seg* segs, int32_t n_segs, segger_stream_t stream);
/* segger_pack_refresh: the compute-dtype copies of fp32 master weights after an optimizer step, all in ONE launch.
 * Per segment: src fp32 [rows, cols] row-major -> dst (bf16 / f16 per `dtype`, [rows, cols] contiguous: the matrix's row
 * window of a row-stacked buffer) and, when dst_t != NULL, its transpose into dst_t[c * ld_t + r] (dst_t already points
 * at the matrix's COLUMN window of the stacked transposed buffer [cols, ld_t]).  dst_f32 != 0: a bias -- `rows` floats
 * copied fp32 -> fp32 (cols, dst_t ignored).  Replaces torch._foreach_copy_ x 2 + segger_transpose_many. */
typedef struct {
  const float* src;
  void* dst;
  void* dst_t;
  int64_t ld_t;
  int32_t rows, cols;
  int32_t dst_f32;
  int32_t reserved_;
} segger_pack_seg;
int segger_pack_refresh(const segger_pack_seg* segs, int32_t n_segs, int32_t dtype, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Prediction head: cosine similarity on tx->bd candidate edges + per-transcript
 * arg-max + assignment.  Replaces torch.cosine_similarity on two gathered
 * [Ep, C] tensors, torch_scatter.scatter_max and the masked fancy-indexing of
 * src/segger/models/lightning_model.py:275-293.
 *   ties -> lowest original edge id (torch_scatter CPU semantics);
 *   transcript without candidate edges -> max_sim 0, max_eid n_edges, seg -1.
 * ---------------------------------------------------------------------- */
typedef struct segger_edge_argmax_args {
  segger_csr by_src;      /* rows = transcripts, col = boundary ids */
  const void* z_src;      /* [n_rows, C] */
  int64_t ld_zs;
  const void* z_dst;      /* [n_cols, C] */
  int64_t ld_zd;
  int32_t channels;
  int32_t dtype;
  float eps;              /* 1e-8 (torch.cosine_similarity) */
  int32_t use_min_similarity;
  float min_similarity;
  const int64_t* dst_index; /* [n_cols] boundary 'index' attribute; NULL = identity */
  float* max_sim;         /* [n_rows] */
  int64_t* max_eid;       /* [n_rows] */
  int64_t* seg_idx;       /* [n_rows] dst_index[col of arg-max] or -1 */
  float* sim;             /* [n_edges] per-edge cosine by ORIGINAL edge id; NULL = skip */
} segger_edge_argmax_args;

int segger_edge_cos_argmax(const segger_edge_argmax_args* args, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Training head: triplet margin loss over tx-belongs-bd edges with sampled
 * negative boundaries.  Replaces 3 gathers + torch.nn.TripletMarginLoss
 * (margin, p=2, eps=1e-6, mean) at src/segger/models/lightning_model.py:182-187
 * and its autograd.
 *   loss = mean_e max(||a-p+eps|| - ||a-n+eps|| + margin, 0)
 * fwd writes partial sums; `loss` receives the mean (loss == NULL: partial sums only, see
 * segger_loss_combine_partials_fwd).  bwd accumulates
 * (atomics: fp32, or packed 16-bit pairs, see grad_*_packed) into grad_a / grad_b, which the caller zero-fills.
 * ---------------------------------------------------------------------- */
typedef struct segger_triplet_args {
  const int64_t* src;     /* [n_edges] anchor rows of z_a */
  const int64_t* pos;     /* [n_edges] positive rows of z_b */
  const int64_t* neg;     /* [n_edges] negative rows of z_b */
  int64_t n_edges;
  const void* z_a;        /* [n_a, C] */
  int64_t ld_za;
  int64_t n_a;
  const void* z_b;        /* [n_b, C] */
  int64_t ld_zb;
  int64_t n_b;
  int32_t channels;
  int32_t dtype;
  float margin;
  float eps;
  float* loss;            /* [1] */
  float grad_scale;       /* bwd: dL/dloss (the 1/n_edges is applied inside) */
  const float* grad_scale_dev; /* bwd: optional DEVICE scalar multiplied into grad_scale (avoids a host sync) */
  void* grad_a;           /* [n_a, C] bwd only: fp32, or `dtype` when grad_a_packed */
  void* grad_b;           /* [n_b, C] bwd only: fp32, or `dtype` when grad_b_packed */
  int32_t grad_a_packed;  /* 1: accumulate with packed 2-channel atomics in the embeddings' 16-bit dtype (half the
                             atomics, no fp32 staging + cast); meant for matrices whose rows collect a handful of
                             terms (transcripts); needs a 16-bit dtype and even C */
  int32_t grad_b_packed;
  float* contrib;         /* bwd, optional: [n_edges, 2, C] fp32.  When given, the z_b side uses NO atomics: triplet e
                             leaves (-dL/d z_b[pos_e], +dL/d z_b[neg_e]) in rows 2e, 2e+1 (zeros when inactive) and the
                             caller sums the rows grouped by boundary with segger_segment_rowsum; grad_b is ignored */
  void* workspace;
  size_t workspace_bytes;
  const int64_t* pos_indptr; /* bwd, optional: [n_b + 1] and ... */
  const int32_t* pos_eid;    /* ... [n_edges]: the triplets grouped by their positive row (for tx-belongs-bd edges this is
                                the by-destination CSR the encoder already built).  When given (separate z_b, fp32
                                grad_b), the positive side of grad_b is a segmented sum over these groups -- written,
                                not accumulated, so grad_b needs no zero-fill -- and only the negatives, which are
                                sampled uniformly and therefore uncontended, use fp32 atomics.  (Positives are the hot
                                rows: a boundary's ~40 edges sit next to each other and hammer one row.) */
  int32_t anchor_unique;     /* bwd, with pos_indptr: 1 = no row of z_a is the anchor of two triplets (tx-belongs-bd: a
                                transcript lies in at most one boundary, heterodata.py:147).  The whole backward is then
                                ONE walk over the groups: the anchor's row of grad_a is STORED (non-anchor rows keep the
                                caller's zeros; later kernels may add to it), the group's positive row is summed in
                                registers and added once, negatives add by fp32 atomics -- grad_b is ACCUMULATED INTO
                                (caller zero-fills it), every embedding row is read once.  C in {32, 64, 96, 128}. */
  int32_t loss_kind;         /* SEGGER_LOSS_TRIPLET (0) or SEGGER_LOSS_BCE: the BCE variant of the segmentation loss
                                (lightning_model.py:190-207), BCEWithLogits over the dot-product logits <a, pos> (label 1)
                                and <a, neg> (label 0), mean over the 2 n_edges logits; margin / eps / contrib unused;
                                grad_b is always accumulated into (caller zero-fills); with pos_indptr + anchor_unique
                                the backward is the same one walk over the groups as for the triplet loss */
  void* grad_a_rows;         /* bwd, optional (triplet loss): [n_a, C] in the format of grad_a.  For triplets whose anchor is
                                their own index (src[e] == e or skipped, n_edges == n_a: loss_tx, where every row anchors one
                                triplet) the anchor's term of triplet e is STORED into row e (zeros when the triplet is
                                inactive or skipped) instead of added atomically; grad_a / grad_b then receive only the
                                positive / negative terms.  The consumer adds the two matrices (segger_l2norm_bwd2). */
} segger_triplet_args;
#define SEGGER_LOSS_TRIPLET 0
#define SEGGER_LOSS_BCE 1

/*
 * segger_loss_combine_fwd / _bwd: the loss combination of LitISTEncoder.get_losses (lightning_model.py:136-149,
 * 210-211: scheduled weights, weighted sum) on DEVICE scalars, one launch each way instead of a chain of 0-dim torch ops:
 *   out[i] = raw[i] * a[i]  (the logged losses; a = per-loss rescaling, e.g. padded -> masked means),
 *   out[n] = sum_i out[i] * b[i]  (b = scheduled weights);    grad_raw[i] = (grad_out[n] * b[i] + grad_out[i]) * a[i].
 * raw / a / b: float[n] on the device, n <= 16; grad_raw feeds grad_scale_dev of the loss kernels' backward.
 */
int segger_loss_combine_fwd(const float* raw, const float* a, const float* b, int32_t n, float* out, segger_stream_t stream);
/* The same with raw[i] = scale[i] * sum(partial[i][0 .. n_partial[i])): segger_triplet_fwd / segger_metric_fwd called with
 * loss == NULL leave their per-block partial sums (segger_triplet_partial_count(n) floats) at the start of their workspace;
 * this launch finishes all of them (in a fixed order) and combines -- one launch instead of one per loss + one.
 * partial / n_partial / scale are HOST arrays of n entries (device pointers inside partial). */
int64_t segger_triplet_partial_count(int64_t n_edges);
int segger_loss_combine_partials_fwd(const float* const* partial, const int64_t* n_partial, const float* scale, const float* a,
                                     const float* b, int32_t n, float* out, segger_stream_t stream);
int segger_loss_combine_bwd(const float* grad_out, const float* a, const float* b, int32_t n, float* grad_raw,
                            segger_stream_t stream);

/*
 * segger_triplet_sample: FastTripletSelector.sample_triplets (src/segger/models/triplet_loss.py:83-125) for all
 * nodes in one launch: per node i with cluster r = lab[i], draw the positive cluster from row r of cdf_pos and the
 * negative cluster from row r of cdf_neg (first column whose cumulative probability >= u, as torch.searchsorted),
 * then the member  members[offsets[c] + floor(u' * counts[c])]  of the drawn cluster c.
 *   lab      [n] int64 cluster id per node; ids >= n_clusters (the "masked out" cluster) get pos = neg = -1
 *   cdf_pos / cdf_neg [n_clusters, n_clusters] fp32 row-wise cumulative distributions
 *   counts / offsets  [n_clusters (+1)] int64, members [n] int64 (nodes grouped by cluster)
 *   uniforms [4, n] fp32 (cluster+, member+, cluster-, member-) or NULL: then U[0,1) comes from a counter-based
 *            generator keyed by (seed + *seed_dev, node, draw) -- same construction as the dropout stream
 *   dists    [n_clusters, n_clusters] fp32 or NULL; when given d_pos / d_neg [n] receive dists[r, cluster of pick]
 */
int segger_triplet_sample(const int64_t* lab, int64_t n, int32_t n_clusters, const float* cdf_pos, const float* cdf_neg,
                          const int64_t* counts, const int64_t* offsets, const int64_t* members,
                          const float* uniforms, uint64_t seed, const uint64_t* seed_dev,
                          const float* dists, int64_t* pos, int64_t* neg, float* d_pos, float* d_neg,
                          segger_stream_t stream);

/*
 * segger_sample_negatives: the negative destinations of the segmentation loss (lightning_model.py:178-180:
 *   dst_neg = (dst_pos + randint(1, n_b)) % n_b ) in one launch:  neg[e] = (pos[e] + 1 + floor(u * (n_b - 1))) % n_b
 * with u from the counter-based generator keyed by (seed + *seed_dev, e); pos[e] < 0 (a padded triplet) gives -1.
 * n_b_dev (optional) overrides n_b with a device value (a captured step padded to a static size); n_b <= 1 gives 0.
 */
int segger_sample_negatives(const int64_t* pos, int64_t n, int64_t n_b, const int64_t* n_b_dev, uint64_t seed,
                            const uint64_t* seed_dev, int64_t* neg, segger_stream_t stream);

/*
 * segger_metric_fwd / _bwd: MetricLoss.forward (src/segger/models/triplet_loss.py:163-204) on sampled triplets,
 *   loss = sum_i w_i * [ (cos(z_i, z_pos_i) - (1 - d_pos_i))^2 + (cos(z_i, z_neg_i) - (1 - d_neg_i))^2 ]
 * with cos(x, y) = sum (x / max(|x|, eps)) * (y / max(|y|, eps)) (torch.cosine_similarity, eps = 1e-8) and w_i the
 * weight of node i (1/n for the reference's plain mean; mask_i / #masked for the masked form).  pos_i / neg_i < 0
 * (or w_i == 0) skip the node.  ~40 torch launches forward and as many backward become one kernel each.
 *   fwd: partial sums in workspace (segger_triplet_workspace_bytes(n)), mean in loss[0].
 *   bwd: grad_z [n, C] fp32, ZERO-FILLED by the caller, receives d loss / d z scaled by grad_scale_dev[0]
 *        (own row: plain add by the owning lanes; positive / negative rows: fp32 atomics).
 */
int segger_metric_fwd(const void* z, int64_t ld_z, int64_t n, int32_t channels, int32_t dtype, const int64_t* pos,
                      const int64_t* neg, const float* d_pos, const float* d_neg, const float* w, float eps,
                      float* loss, void* workspace, size_t workspace_bytes, segger_stream_t stream);
int segger_metric_bwd(const void* z, int64_t ld_z, int64_t n, int32_t channels, int32_t dtype, const int64_t* pos,
                      const int64_t* neg, const float* d_pos, const float* d_neg, const float* w, float eps,
                      const float* grad_scale_dev, float* grad_z, segger_stream_t stream);

size_t segger_triplet_workspace_bytes(int64_t n_edges);
int segger_triplet_fwd(const segger_triplet_args* args, segger_stream_t stream);
int segger_triplet_bwd(const segger_triplet_args* args, segger_stream_t stream);

/*
 * segger_loss_head_fwd / _bwd: LitISTEncoder.get_losses after the sampling (lightning_model.py:151-213: loss_tx =
 * TripletLoss, loss_bd = MetricLoss (models/triplet_loss.py:128-204), loss_sg = TripletMarginLoss or BCEWithLogits on the
 * tx-belongs-bd edges (:167-207), weighted sum :210-211) as ONE launch each way (csrc/loss_head.hip).  Same arithmetic as
 * segger_triplet_* / segger_metric_* / segger_loss_combine_*, which remain for other shapes.
 *   loss_tx triplets are (t, tx_pos[t], tx_neg[t]), t < n_tx (rows of z_tx; tx_pos[t] < 0 skips t; mean over n_tx);
 *   loss_bd as segger_metric_fwd over the rows of z_bd;  loss_sg over n_sg triplets (sg_src -> z_tx, sg_pos / sg_neg -> z_bd;
 *   sg_pos < 0 skips; mean over n_sg, or over 2 n_sg logits for SEGGER_LOSS_BCE).
 *   out[0..2] = a[i] * loss_i, out[3] = sum_i b[i] out[i]  (a, b: float[3] on the device, as segger_loss_combine_fwd).
 * Forward, with tx_w / tx_state / tx_next / tx_hot_id / tx_hot_acc given (a training step): per loss_tx triplet the reciprocal
 *   distances of ACTIVE triplets (tx_w [n_tx, 2], 0 = inactive) and the chains of contributions per target row: tx_state
 *   int32 [2 n_tx + 4] = per row (chain head, contribution count), then the hot-row counter -- the CALLER ZERO-FILLS it
 *   before every forward launch (a chain walk is bounded whatever it holds: a stale buffer gives wrong numbers, never a
 *   spinning kernel); tx_next int32 [2 n_tx]; a row that receives more than 64 contributions (skewed draws: few members of a
 *   much-drawn cluster in the batch) is "hot": tx_hot_id int32 [n_tx + segger_loss_head_max_hot_rows(n_tx)] and tx_hot_acc fp32 [segger_loss_head_max_hot_rows(n_tx),
 *   C] hold its accumulator (no initialisation needed).  With grad_bd given the launch zero-fills it; with grad_out
 *   (float[4], d / d out) given it also writes grad_raw[3], the scale factors of the three backward terms
 *   (segger_loss_combine_bwd's result).
 * Backward: grad_tx [n_tx, C] (dtype of the embeddings) is WRITTEN, every row once, no atomics: row r = its anchor term of
 *   loss_tx + the positive / negative terms of the triplets chained to r + the anchor term of the segmentation triplet
 *   sg_of_tx[r] (int32 [n_tx], -1 = none: requires that no transcript anchors two segmentation triplets; NULL = the
 *   segmentation loss contributes nothing to grad_tx, the caller adds it); with y_tx given (z_tx = y_tx / max(|y_tx|,
 *   norm_eps) row-wise) the row is pushed through that normalisation's backward and grad_tx is d / d y_tx.  Hot rows are
 *   accumulated with fp32 atomics by the groups of the contributing triplets and finished by the last contributor.
 *   grad_bd [n_bd, C] fp32 is ACCUMULATED INTO (zero-filled by the forward): metric loss, segmentation positives (summed
 *   per boundary over sg_pos_indptr [n_bd + 1] / sg_pos_eid [n_sg], the triplets grouped by positive row) and negatives.
 * workspace: segger_loss_head_workspace_bytes() (per-block partial sums; the forward is TWO launches: the loss kernel and a
 *   one-workgroup launch that adds the partial sums in a fixed order -- a last-block-by-ticket form paid a whole-L2
 *   write-back per block for its device-scope release: 0.76 of 0.90 ms at 10^6 rows); ticket: unused (kept for layout).
 *   C in {32, 64, 128}.  Worth it below ~10^5 transcript rows (a captured 1M-edge step); at 10^6 rows the forward's chain
 *   atomics (4 returning atomics per triplet) make it slower than the kernel-by-kernel head (profiles/r04_loss_head_modes_c2.txt).
 */
#define SEGGER_LOSS_HEAD_DEFER_FINISH 1   /* in reserved_: with grad_out given, the forward leaves its partial sums and the
                                             backward launch (one extra workgroup) finishes the losses into `out`; both calls
                                             get the same workspace, out and grad_out: a captured training step's form */
typedef struct segger_loss_head_args {
  const void* z_tx; int64_t ld_ztx; int64_t n_tx;
  const void* z_bd; int64_t ld_zbd; int64_t n_bd;
  int32_t channels, dtype;
  const int64_t* tx_pos; const int64_t* tx_neg; float tx_margin, tx_eps;
  const int64_t* bd_pos; const int64_t* bd_neg; const float* bd_dpos; const float* bd_dneg; const float* bd_w; float bd_eps;
  int32_t sg_kind;
  const int64_t* sg_src; const int64_t* sg_pos; const int64_t* sg_neg; int64_t n_sg; float sg_margin, sg_eps;
  const int64_t* sg_pos_indptr; const int32_t* sg_pos_eid; const int32_t* sg_of_tx;
  const float* a; const float* b; const float* grad_out; float* out; float* grad_raw;
  float* tx_w; int32_t* tx_state; int32_t* tx_next; int32_t* tx_hot_id; float* tx_hot_acc;
  const void* y_tx; int64_t ld_ytx; float norm_eps; int32_t reserved_;
  void* grad_tx; int64_t ld_gtx; float* grad_bd;
  void* workspace; size_t workspace_bytes; int32_t* ticket;
} segger_loss_head_args;
size_t segger_loss_head_workspace_bytes(int64_t n_tx, int64_t n_bd, int64_t n_sg);
int64_t segger_loss_head_max_hot_rows(int64_t n_tx);
int segger_loss_head_supported(int32_t channels, int32_t dtype);
int segger_loss_head_fwd(const segger_loss_head_args* args, segger_stream_t stream);
int segger_loss_head_bwd(const segger_loss_head_args* args, segger_stream_t stream);

/*
 * segger_loss_head_ordered_fwd / _bwd: the same head with an ORDERED backward (csrc/loss_head_ordered.hip) -- the
 * deterministic training mode.  For given inputs (the embeddings, tx_pos / tx_neg / bd_pos / bd_neg / sg_*, the weights,
 * grad_out) every byte of out, grad_tx and grad_bd is a function of those inputs alone: no float atomic is on the
 * route (the radix sort's integer atomics cannot show in a keys-only result), nothing depends on the scheduling or on the grid.  Same struct and the same meaning of every
 * field, except:
 *   tx_state, tx_next, tx_hot_id, tx_hot_acc must be NULL (there are no chains and no hot rows); tx_w [n_tx, 2] alone says
 *   "a training step", and nothing needs zero-filling by the caller;  grad_bd [n_bd, C] fp32 is WRITTEN by the backward,
 *   every row once (the forward does not touch it);  workspace: segger_loss_head_ordered_workspace_bytes(), 256-byte
 *   aligned, the SAME buffer in both calls (the forward leaves the sorted contribution keys and the rows' segment offsets
 *   in it): sized from the three counts alone, so a captured step allocates it with its other static buffers.
 * Forward: segger_loss_head_fwd's loss kernel (+ finish, or neither with DEFER_FINISH), whose partial sums are added in a
 *   fixed order on both paths; with tx_w given, then one key per possible contribution (2 n_tx + 2 n_bd + n_sg keys:
 *   target row, role, contributor id; an inactive one sorts behind every row), one keys-only radix sort, one binary search
 *   per row for its segment.  No allocation, no host wait: all of it can be captured.
 * Backward, THE ORDER of every sum (fp32, rounded once per row):
 *   transcript row r: (1) its own anchor term of loss_tx; (2) the terms of the triplets that name r as positive, by
 *     ascending triplet id; (3) of those that name it as negative, by ascending triplet id; (4) the anchor term of its
 *     segmentation triplet sg_of_tx[r]; then the row normalisation's backward when y_tx is given.  With at most 64 terms
 *     under (2) + (3) they are added one after the other onto (1).  With more, term k of that list (k from 0, positives
 *     first) is added to partial sum P[k mod 16], each P starting at zero and adding in list order, and the row is
 *     ((1) + P[0] + ... + P[15]) + (4), left to right.
 *   boundary row j: (1) its own loss_bd term, + P[0] + ... + P[15] left to right, where the list that feeds P[k mod 16]
 *     is: (2) the loss_bd terms of the nodes that name j as positive, by ascending node; (3) as negative, by ascending
 *     node; (4) the sampled loss_sg negatives that hit j, by ascending triplet id; and then, k counting from 0 again,
 *     (5) j's own loss_sg positives in the order of sg_pos_indptr / sg_pos_eid.
 *   Which of the two transcript forms a row takes is decided by the length of its list: the order is a function of the
 *   indices only.  Every loop is bounded by the number of keys and every id read from the workspace is checked against
 *   its matrix: a stale workspace gives wrong numbers, never a spinning kernel or an access outside the buffers.
 */
size_t segger_loss_head_ordered_workspace_bytes(int64_t n_tx, int64_t n_bd, int64_t n_sg);
int segger_loss_head_ordered_fwd(const segger_loss_head_args* args, segger_stream_t stream);
int segger_loss_head_ordered_bwd(const segger_loss_head_args* args, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Positional embedder, stage 1: per-graph min / max of node positions.
 * Replaces the Python loop over graphs in Positional2dEmbedder.forward
 * (src/segger/models/ist_encoder.py:66-73: one boolean mask, two reductions and a
 * host sync per graph).
 *   pos   : [n, 2] fp32 ;  batch : [n] int64 graph id per node, or NULL (one graph)
 *   mins / maxs : [n_graphs, 2] fp32 ; a graph without nodes gets (0, 0) as in the
 *   reference; ids outside [0, n_graphs) are ignored.
 * segger_segment_minmax_ex, flags: SEGGER_MINMAX_INITIALISED = the caller has already filled mins with +inf and maxs with
 *   -inf (e.g. in its staging launch); SEGGER_MINMAX_KEEP_EMPTY = leave (+inf, -inf) for graphs without nodes (a consumer
 *   that only looks up the graphs of existing nodes never reads them): one launch instead of three.
 * ---------------------------------------------------------------------- */
#define SEGGER_MINMAX_INITIALISED 1
#define SEGGER_MINMAX_KEEP_EMPTY 2
int segger_segment_minmax_ex(const float* pos, const int64_t* batch, int64_t n, int64_t n_graphs, float* mins, float* maxs,
                             int32_t flags, segger_stream_t stream);
int segger_segment_minmax(const float* pos, const int64_t* batch, int64_t n, int64_t n_graphs,
                          float* mins, float* maxs, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Tall-skinny projection on the matrix cores (v_mfma_f32_32x32x16):
 *     y[n, m_out] = x[n, k_in] * w[m_out, k_in]^T (+ bias)
 * Replaces the cuBLAS GEMMs behind PyG's Linear for GATv2Conv.lin_l / lin_r
 * (constructed at src/segger/models/ist_encoder.py:111-124), HeteroDictLinear
 * (ist_encoder.py:282-286,328) and, called with w = W^T, their data gradients.
 * Every workgroup owns 128 rows and ALL m_out columns, so x is read from HBM once.  From ~2*10^5 rows on, for
 * k_in in {64, 128} and m_out in {64, 128, 384}, one persistent workgroup per CU keeps the whole w in LDS and its waves
 * walk 32-row tiles independently (same arithmetic, bit-identical results).
 *   dtype: SEGGER_BF16 / SEGGER_F16 (x, w, y); bias fp32 or NULL; fp32 accumulation.
 *   k_in in {64, 128, 256, 384}; m_out a multiple of 64; w contiguous [m_out, k_in].
 * segger_linear_supported() tells the host whether a shape is covered (others go to
 * the vendor GEMM library).
 * ---------------------------------------------------------------------- */
int segger_linear_supported(int32_t k_in, int32_t m_out, int32_t dtype);
int segger_linear_fwd(const void* x, int64_t ldx, const void* w, const float* bias, void* y, int64_t ldy,
                      int64_t n_rows, int32_t k_in, int32_t m_out, int32_t dtype, segger_stream_t stream);
/* segger_linear_fwd_silu_grad: y = (x @ w^T) * silu'(gate), gate [n_rows, m_out] in `dtype`: the data gradient through
 * Linear -> SiLU (the positional MLP, ist_encoder.py:45-49) with torch's separate silu_backward pass folded into the
 * GEMM epilogue.  k_in = 64. */
int segger_linear_fwd_silu_grad(const void* x, int64_t ldx, const void* w, const void* gate, int64_t ld_gate, void* y,
                                int64_t ldy, int64_t n_rows, int32_t k_in, int32_t m_out, int32_t dtype,
                                segger_stream_t stream);
/* segger_linear_fwd_rowbias: the same with  y[row, :] += rowbias[rowidx[row], :]  added in the epilogue (table
 * [n_ids, ld_rb >= m_out] in `dtype`, 16-byte aligned rows, added in fp32; int32 ids in range -- not checked): the gene-embedding half of the first layer's projections
 * collapses to a per-gene table T = gelu(E) Wa^T + b ([n_genes, 384]), so the GEMM runs over the positional half only
 * (K 256 -> 128) and gelu(cat(E[g], pe)) is never materialised (ist_encoder.py:312-325 + GATv2Conv.lin_l / lin_r). */
int segger_linear_fwd_rowbias(const void* x, int64_t ldx, const void* w, const float* bias, const void* rowbias,
                              int64_t ld_rb, const int32_t* rowidx, void* y, int64_t ldy, int64_t n_rows, int32_t k_in,
                              int32_t m_out, int32_t dtype, segger_stream_t stream);

/* segger_linear_wgrad_f32_split: segger_linear_wgrad for fp32 storage on the bf16 matrix pipe (both operands split three ways,
 * six partial products; csrc/linear_f32_split.hip) -- the weight gradient autograd forms as `grad.t() @ x` for the nn.Linear
 * maps of ist_encoder.py:111-124,282-286.  Same arguments, workspace (segger_linear_wgrad_workspace_bytes) and deterministic
 * slab-order sums as segger_linear_wgrad; error within the exact-fp32 kernel's own, not bit-identical to it. */
/* segger_linear_fwd_f32_act: y = x @ W^T + b AND y_act = act(y) (act_kind 1 = GELU, 2 = SiLU) from one kernel at fp32 storage:
 * the pre-activation the backward keeps and the activation the next layer reads (the positional MLP's Linear -> SiLU and its
 * output's GELU, ist_encoder.py:43-49,320) without torch's separate elementwise pass.  Exact-fp32 kernel, k_in 64 / 128 / 256. */
int segger_linear_fwd_f32_act(const float* x, int64_t ldx, const float* w, const float* bias, float* y, int64_t ldy,
                              float* y_act, int64_t ld_yact, int32_t act_kind, int64_t n_rows, int32_t k_in, int32_t m_out,
                              segger_stream_t stream);
/* segger_linear_fwd_f32_gate: y = (x @ W^T) * act'(gate) at fp32 storage -- the data gradient through GELU (gate_kind 1) or
 * SiLU (2) with torch's separate gelu_backward / silu_backward pass folded into the GEMM epilogue (ist_encoder.py:47,320:
 * the positional MLP's SiLU, the GELU on the first layer's input).  w_is_planes != 0: W as the three bf16 planes of
 * segger_f32_split_planes (shapes of segger_linear_fwd_f32_split_supported); else W [m_out, k_in] fp32 on the exact-fp32
 * kernel (k_in 64 / 128 / 256).  gate [n_rows, ld_gate >= m_out] fp32. */
int segger_linear_fwd_f32_gate(const float* x, int64_t ldx, const void* w, int32_t w_is_planes, const float* gate,
                               int64_t ld_gate, int32_t gate_kind, float* y, int64_t ldy, int64_t n_rows, int32_t k_in,
                               int32_t m_out, segger_stream_t stream);
/* segger_f32_split_planes: planes [3][rows * cols] bf16 (hi, mid, lo: they add up to the fp32 number exactly) of w [rows, cols]
 * fp32 row-major, laid out as w or, transpose != 0, as w^T [cols, rows]: the weight operand of segger_linear_fwd_f32_split,
 * refreshed after every optimizer step. */
int segger_f32_split_planes(const float* w, int32_t rows, int32_t cols, int32_t transpose, void* planes, segger_stream_t stream);
/* ... for up to SEGGER_PLANES_MAX_JOBS matrices in ONE launch (every fp32 weight pack of a model after an optimizer step:
 * nn.Linear / GATv2Conv.lin_l / lin_r weights of ist_encoder.py:111-124,261,282-286); per job the arguments of
 * segger_f32_split_planes. */
#define SEGGER_PLANES_MAX_JOBS 32
typedef struct segger_planes_job {
  const float* w;      /* [rows, cols] fp32, contiguous */
  int32_t rows, cols;
  int32_t transpose;   /* non-zero: planes of w^T */
  int32_t reserved_;
  void* planes;        /* bf16 [3][rows * cols] */
} segger_planes_job;
int segger_f32_split_planes_many(const segger_planes_job* jobs, int32_t n_jobs, segger_stream_t stream);
int segger_linear_wgrad_f32_split_supported(int32_t m_out, int32_t k_in);
int segger_linear_wgrad_f32_split(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, int64_t n_rows, int32_t m_out,
                                  int32_t k_in, float* grad_w, float* grad_b, void* workspace, size_t workspace_bytes,
                                  segger_stream_t stream);

/* segger_gene_table_fwd/bwd: the per-gene table of segger_linear_fwd_rowbias and everything that flows back through it,
 * one launch each way (csrc/gene_table.hip) -- torch formed it with ~25 small launches per step (gelu, cat, vendor GEMMs,
 * slice gradients).  The first hetero layer projects gelu(cat(E[gene], pe)) with n_w (<= 4) stacked nn.Linear maps
 * w[i] [m[i], ld_w[i] >= 2 D] fp32 (GATv2Conv.lin_l / lin_r, ist_encoder.py:111-124), bias b[i] [m[i]] or NULL; M = sum m[i].
 *   fwd: tab [n_genes, ld_tab >= M] = gelu(E) Wa^T + b, Wa = w[:, 0:D], in `dtype`; wc [M, D] = w[:, D:2D] and wc_t [D, M]
 *        its transpose, both in `dtype` (either may be NULL).
 *   bwd: from g_tab [n_genes, M] fp32 (rows of dY summed by gene) and g_wc [M, D] fp32 (dWc of the positional GEMM; NULL:
 *        right halves left untouched): g_table [n_genes, D] = gelu'(E) * (g_tab Wa) (NULL to skip); g_w[i] [m[i], 2 D]
 *        contiguous fp32 = [g_tab^T gelu(E) | g_wc] rows of weight i; g_b[i] [m[i]] = column sums of g_tab (NULL to skip). */
typedef struct segger_gene_table_args {
  const float* table; int32_t n_genes; int32_t D; int32_t n_w; int32_t dtype;
  const float* w[4]; int64_t ld_w[4]; int32_t m[4]; const float* b[4];
  void* tab; int64_t ld_tab; void* wc; void* wc_t;                    /* forward outputs */
  const float* g_tab; const float* g_wc;                              /* backward inputs */
  float* g_table; float* g_w[4]; float* g_b[4];                       /* backward outputs */
} segger_gene_table_args;
int segger_gene_table_fwd(const segger_gene_table_args* args, segger_stream_t stream);
int segger_gene_table_bwd(const segger_gene_table_args* args, segger_stream_t stream);

/* segger_linear_fwd_f32_split: the fp32-storage projection on the bf16 matrix pipe -- every fp32 operand as the sum of three
 * bf16 numbers, the product as its six leading partial products, each exact in the MFMA's fp32 accumulator
 * (csrc/linear_f32_split.hip).  An OPT-IN alternative to segger_linear_fwd's exact-fp32 kernel for the same nn.Linear call
 * sites (ist_encoder.py:111-124,282-286 under a default fp32 Trainer, cli/segment.py:400-405): error ~2^-22 relative to
 * sum |x||w| instead of fp32 rounding only, at 6/16 of the bf16 MFMA rate instead of the 157 TFLOP/s fp32 pipe.
 *   x [n, k_in] fp32, y [n, m_out] fp32 (16-byte aligned rows); w3 = bf16 [3][m_out][k_in]: hi = bf16(w), mid = bf16(w - hi),
 *   lo = bf16(w - hi - mid).  Covered: k_in 128 with m_out a multiple of 64; k_in 384 with m_out 128 (dX = dY W on W^T planes).
 * RANGE: not range-equivalent to the exact kernel.  bf16 has fp32's exponent range but rounds up at the top: an operand with
 * |v| > 0x7F7F8000 as fp32 bits (3.3895e38: within 2^-9 of FLT_MAX) rounds its hi plane to +-inf and the result is NaN
 * (inf - inf in the mid plane) where the exact kernel stays finite; sub-normal operands lose the planes below 2^-133.  Node
 * features behind a GELU / L2 normalisation are nowhere near either end; callers that cannot promise it select the exact
 * kernels (host side: SEGGER_AMD_F32_EXACT=1 / ops.F32_SPLIT = False -- the active mode is recorded on bench.py's line,
 * f32.projections). */
int segger_linear_fwd_f32_split_supported(int32_t k_in, int32_t m_out);
int segger_linear_fwd_f32_split(const float* x, int64_t ldx, const void* w3, const float* bias, float* y, int64_t ldy,
                                int64_t n_rows, int32_t k_in, int32_t m_out, segger_stream_t stream);
/* ... with y[row, :] += rowbias[rowidx[row], :] in the epilogue (fp32 table [n_ids, ld_rb >= m_out]; no bias): the fp32 form
 * of segger_linear_fwd_rowbias on the split kernel. */
int segger_linear_fwd_f32_split_rowbias(const float* x, int64_t ldx, const void* w3, const float* rowbias, int64_t ld_rb,
                                        const int32_t* rowidx, float* y, int64_t ldy, int64_t n_rows, int32_t k_in,
                                        int32_t m_out, segger_stream_t stream);

/* segger_linear_fwd_pair: two such projections with the same k_in and dtype as ONE launch -- a hetero layer projects its
 * transcripts ([lin_l | lin_r | lin_l], ist_encoder.py:109-134 through HeteroConv) and its ~10^2-10^3 boundaries (lin_r)
 * in the same step, and lin_last maps both node types (ist_encoder.py:282-286,328); the small one's blocks ride in the
 * large one's grid instead of paying a launch of their own (a large `a` takes its persistent resident-W launch and `b` its
 * own; fp32: two launches).  Same arithmetic as segger_linear_fwd, bit-identical results. */
typedef struct segger_linear_args {
  const void* x; int64_t ldx; const void* w; const float* bias; void* y; int64_t ldy; int64_t n_rows; int32_t m_out;
  int32_t reserved_;
} segger_linear_args;
int segger_linear_fwd_pair(const segger_linear_args* a, const segger_linear_args* b, int32_t k_in, int32_t dtype,
                           segger_stream_t stream);
/* ... and with an input width per side (a first layer's two data gradients dX = dY W read 384 and 128 columns of dY): one
 * launch for (k_a, k_b) = (384, 128) or equal widths, two otherwise. */
int segger_linear_fwd_pair_k(const segger_linear_args* a, int32_t k_a, const segger_linear_args* b, int32_t k_b,
                             int32_t dtype, segger_stream_t stream);

/*
 * segger_linear_wgrad: the parameter gradients of the same projections,
 *     grad_w[M, K] = dY[n, M]^T * X[n, K]      grad_b[M] = sum_n dY[n, :]       (fp32 outputs)
 * i.e. what torch autograd computes for nn.Linear / PyG Linear (lin_l, lin_r, lin_last, the positional MLP;
 * src/segger/models/ist_encoder.py:44-48,111-124,261,282-286) as `grad.t() @ x` and `grad.sum(0)`.
 * One pass over dY and X on the matrix cores: row slabs per workgroup, the whole [M, K] accumulator in
 * registers, transposed operand reads from LDS (ds_read_b64_tr_b16), deterministic slab-order reduction.
 *   dy [n_rows, m_out] row stride ld_dy, x [n_rows, k_in] row stride ld_x (elements; 16-byte aligned rows)
 *   covered: m_out in {64,128,192,384}, k_in in {64,128,256}, bf16 / f16 (segger_linear_wgrad_supported)
 *   grad_b may be NULL; workspace >= segger_linear_wgrad_workspace_bytes(n_rows, m_out, k_in)
 */
int segger_linear_wgrad_supported(int32_t m_out, int32_t k_in, int32_t dtype);
size_t segger_linear_wgrad_workspace_bytes(int64_t n_rows, int32_t m_out, int32_t k_in);
int segger_linear_wgrad(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, int64_t n_rows,
                        int32_t m_out, int32_t k_in, int32_t dtype, float* grad_w, float* grad_b,
                        void* workspace, size_t workspace_bytes, segger_stream_t stream);
/* segger_linear_wgrad_dx: the WHOLE backward of one projection in one pass over dY:
 *     grad_w, grad_b as above, and    dx[n, K] = dY[n, M] * W[M, K]
 * (autograd's `grad @ weight` for the same nn.Linear / PyG Linear call sites).  dY [n, 3*HC] of the stacked
 * lin_l | lin_r | lin_l projections is the widest matrix of a layer's backward; the separate data-gradient GEMM
 * (segger_linear_fwd on W^T) read it a second time.  w_t = W^T, [k_in, m_out] contiguous in `dtype`; dx row stride
 * ld_dx (elements, 16-byte aligned rows); covered: k_in == 128, m_out in {64,128,192,384}, bf16 / f16
 * (segger_linear_wgrad_dx_supported); workspace as for segger_linear_wgrad.
 * gelu_gate (optional, [n, k_in] in `dtype`, row stride ld_gate): dx[row, c] *= gelu'(gelu_gate[row, c]) in the epilogue
 * -- the projection's input was gelu(gate) (ISTEncoder's GELU on the concatenated first-layer input,
 * ist_encoder.py:320): the gradient leaves as d / d gate without an elementwise pass of its own; covered for m_out in
 * {128, 384} (segger_linear_wgrad_dx_gate_supported); NULL = plain dX. */
int segger_linear_wgrad_dx_supported(int32_t m_out, int32_t k_in, int32_t dtype);
int segger_linear_wgrad_dx_gate_supported(int32_t m_out, int32_t k_in, int32_t dtype);
int segger_linear_wgrad_dx(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, const void* w_t, int64_t n_rows,
                           int32_t m_out, int32_t k_in, int32_t dtype, float* grad_w, float* grad_b, void* dx,
                           int64_t ld_dx, const void* gelu_gate, int64_t ld_gate, void* workspace, size_t workspace_bytes,
                           segger_stream_t stream);
/* segger_linear_wgrad_pair: the backward passes of TWO projections with the same k_in and dtype as one launch -- what
 * segger_linear_fwd_pair is to the forward: a hetero layer's transcript-side and boundary-side projections, lin_last of both
 * node types; the small side's one or two workgroups ride in the large side's grid.  With w_t / dx given on both sides the
 * one-pass form (segger_linear_wgrad_dx), with both NULL the weight / bias gradients only (segger_linear_wgrad).  Same
 * arithmetic and workspaces as the single calls (bit-identical results); shape pairs without a paired kernel, fp32 and
 * empty sides run as two launches. */
typedef struct segger_wgrad_args {
  const void* dy; int64_t ld_dy; const void* x; int64_t ld_x; const void* w_t; int64_t n_rows; int32_t m_out; int32_t reserved_;
  float* grad_w; float* grad_b; void* dx; int64_t ld_dx; void* workspace; size_t workspace_bytes;
} segger_wgrad_args;
int segger_linear_wgrad_pair(const segger_wgrad_args* a, const segger_wgrad_args* b, int32_t k_in, int32_t dtype,
                             segger_stream_t stream);

/*
 * Deferred partial sums.  segger_linear_wgrad / _wgrad_dx / segger_posmlp_wgrad and segger_gatv2_bwd finish with a small
 * kernel that sums per-workgroup partials from their workspace into grad_w / grad_b / grad_att / grad_bias.  Between
 *     segger_reductions_defer_begin()  ...  segger_reductions_flush(stream)
 * (process-wide: autograd queues from its own device thread) those sums are queued instead of launched and the flush runs them
 * all as ONE grid (two when a sum has more than 128 partials: those fold into 32 groups first) -- autograd hands every parameter gradient of a backward pass (ist_encoder.py:289-333 under
 * lightning_model.py:215-237) to the optimizer at the same time anyway.  Contract while deferring: the outputs are
 * undefined and the workspaces must stay untouched until the flush has been enqueued on the same stream (or one
 * ordered after the producers); at most 56 sums are queued, further ones run immediately.  The table travels as a
 * kernel argument: no allocation, no synchronisation, capturable.  segger_reductions_pending(): queued sums, -1 when
 * not deferring.
 */
int segger_reductions_defer_begin(void);
int segger_reductions_pending(void);
int segger_reductions_flush(segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Encoder front end / tail as fused row-wise kernels.
 *
 * segger_posfreq: Positional2dEmbedder up to the MLP input
 *   (src/segger/models/ist_encoder.py:74 normalisation, :22-31,:51-55 sinusoid):
 *   out[(n*2 + c), :] = [cos(p f_j) | sin(p f_j)], p = (pos[n,c] - mins[g,c]) / (maxs[g,c] - mins[g,c] + eps),
 *   f_j = exp(-ln(max_period) * j / (freq_dim/2)), g = batch[n] (0 when batch is NULL); out is [2n, freq_dim] in `dtype`.
 *
 * segger_embed_gelu_fwd/bwd: x0 = gelu(cat(table[ids], pe)) (ist_encoder.py:312-320 for the 'tx' type):
 *   table fp32 [n_rows_table, D] (nn.Embedding weight), ids int32 [n], pe [n, D] -> x0 [n, 2D].
 *   bwd: gpe = gx0[:, D:] * gelu'(pe); gtable (optional, NULL to skip) = gelu'(table) * sum over the rows of each
 *   id of gx0[:, :D].  The rows come GROUPED BY ID: gene_ptr int64 [n_rows_table + 1] / gene_rows int32 [n] are the
 *   indptr / col arrays of segger_csr_from_coo(row = ids, col = 0..n-1) (one sort per batch); the sum is a
 *   deterministic two-stage segmented reduction (no atomics).  D % 8 == 0, D <= 2048.
 *
 * segger_l2norm_fwd/bwd: torch.nn.functional.normalize(dim=-1, eps) (ist_encoder.py:331-332) and its gradient;
 *   channels in {8, 16, 32, 64, 128}.
 *
 * segger_colsum: out[c] = sum_n x[n, c] in fp32 -- the bias gradient of every nn.Linear / PyG Linear on the path
 *   (lin_l / lin_r of GATv2Conv, ist_encoder.py:111-124; pos-embedding MLP :45-49; lin_last :282-286), which autograd
 *   computes as grad_output.sum(0).  cols % 8 == 0, cols <= 2048; deterministic (two-stage, no atomics).
 * ---------------------------------------------------------------------- */
int segger_posfreq(const float* pos, const int64_t* batch, const float* mins, const float* maxs, int64_t n,
                   int32_t freq_dim, float eps, float max_period, void* out, int32_t dtype, segger_stream_t stream);
/*
 * segger_posmlp_fwd: the whole Positional2dEmbedder (ist_encoder.py:33-79) in one kernel -- normalisation, the
 * 256-wide sinusoid, Linear(256 -> 64), SiLU, Linear(64 -> 64) -- with the sinusoid features generated in registers as
 * MFMA operand fragments instead of written to / read from HBM (segger_posfreq + two segger_linear_fwd otherwise).
 *   w0 [64, 256], w2 [64, 64] row-major in `dtype` (bf16 / f16), b0 / b2 fp32 [64]
 *   pe   [2n, 64] in `dtype` (= the embedder's [n, 128] output, x half then y half per node)
 *   z1, h1 [2n, 64] in `dtype`, pn [2n] fp32: the pre-activation of the first layer, its SiLU and the normalised
 *        coordinate per row, stored for the backward; all NULL for inference; h1 may be NULL on its own
 *        (segger_posmlp_bwd recomputes it from z1).
 *   gelu != 0: pe receives gelu(embedder output) -- the positional half of ISTEncoder's gelu(cat(...)),
 *        ist_encoder.py:324-325 -- and, when training, pe_pre [2n, 64] the output itself (for gelu'); else pe_pre NULL.
 * segger_posmlp_wgrad: dW0 [64, 256] = dz1^T F and db0 [64] = sum dz1 with F regenerated from pn inside the weight-
 *   gradient kernel (one float per row read instead of a 512-byte feature row); workspace as
 *   segger_linear_wgrad_workspace_bytes(n_rows, 64, 256); n_rows = 2n.
 * segger_posmlp_bwd: the embedder's whole backward from ONE read of g = d loss / d pe ([n_rows = 2n, 64], row stride
 *   ld_g): dW2 = g^T SiLU(z1), db2 = sum g, dz1 = (g W2) * SiLU'(z1) (kept on the chip), dW0 = dz1^T F(pn), db0 =
 *   sum dz1 -- autograd's two `grad.t() @ x`, two `grad.sum(0)`, the `grad @ W` and the SiLU backward of
 *   ist_encoder.py:45-49, 76-79.  w2_t = W2^T [64, 64] row-major in `dtype`; outputs fp32; workspace
 *   segger_posmlp_bwd_workspace_bytes(n_rows); deterministic (per-workgroup partials summed in order).
 * segger_posmlp_bwd_pair: the same for TWO row sets in one launch and one sum of partials -- ISTEncoder embeds the
 *   transcripts' and the boundaries' positions with the same Positional2dEmbedder (reference ist_encoder.py:314-318), so
 *   its four parameters receive ONE gradient (autograd would add the two calls' gradients with four more launches).
 *   Either side may be empty (n_rows 0, pointers ignored); workspace segger_posmlp_bwd_pair_workspace_bytes(n_a, n_b).
 * Covered: frequency_embedding_size 256, hidden_size 128 (segger's in_channels default): segger_posmlp_supported.
 */
int segger_posmlp_supported(int32_t freq_dim, int32_t dim, int32_t dtype);
/*
 * segger_posenc_poly_*: the first Linear of Positional2dEmbedder (ist_encoder.py:45-49 `mlp[0]` applied to the sinusoid of
 * :22-31) at fp32 storage WITHOUT the [2n, freq_dim] feature matrix and without a GEMM.  The embedder's argument is a min-max
 * NORMALISED coordinate p in [0, 1] (:62-64, :74) and every frequency is <= 1, so |w_j p| <= 1: cos / sin equal their Taylor
 * series through p^12 to 1/13! = 1.6e-10, and the sum over the features can be taken first:
 *   z1[row, m] = sum_{d=0..12} coef[m, d] p^d,   coef[m, d] = [d = 0] b0[m] + (-1)^floor(d/2)/d! sum_j W0[m, (d odd ? half : 0) + j] w_j^d
 * segger_posenc_poly_coef: coef [dim][16] fp32 (13 terms + padding) from W0 [dim, freq_dim] / b0 (NULL: none), in float64;
 *   once per step.
 * segger_posenc_poly_fwd: z1 [2n, dim] fp32 (row = 2 * node + axis), optionally h1 = SiLU(z1) and pn [2n] (the normalised
 *   coordinate, all the weight gradient needs); exact fp32 FMA arithmetic.
 * segger_posenc_poly_wgrad: dW0 [dim, freq_dim] = dz1^T F and db0 [dim] = sum dz1 as  M V^T  with the 13 moments
 *   M[m, d] = sum_rows dz1[row, m] pn[row]^d (fp32 per lane, float64 across workgroups, fixed order: deterministic) and V
 *   the features' Taylor coefficients; dz1 [n_rows, dim] fp32 (row stride ld); workspace
 *   segger_posenc_poly_wgrad_workspace_bytes(n_rows, dim).
 * Covered: dim 32 / 64 / 128, even freq_dim <= 4096 (segger: 64, 256), max_period > 1: segger_posenc_poly_supported.
 */
int segger_posenc_poly_supported(int32_t freq_dim, int32_t dim);
int segger_posenc_poly_coef(const float* w0, const float* b0, int32_t freq_dim, int32_t dim, float max_period, float* coef,
                            segger_stream_t stream);
int segger_posenc_poly_fwd(const float* pos, const int64_t* batch, const float* mins, const float* maxs, int64_t n, float eps,
                           const float* coef, int32_t dim, float* z1, float* h1, float* pn, segger_stream_t stream);
size_t segger_posenc_poly_wgrad_workspace_bytes(int64_t n_rows, int32_t dim);
int segger_posenc_poly_wgrad(const float* dz1, int64_t ld, const float* pn, int64_t n_rows, int32_t freq_dim, int32_t dim,
                             float max_period, float* grad_w0, float* grad_b0, void* workspace, size_t workspace_bytes,
                             segger_stream_t stream);
int segger_posmlp_fwd(const float* pos, const int64_t* batch, const float* mins, const float* maxs, int64_t n, float eps,
                      float max_period, const void* w0, const float* b0, const void* w2, const float* b2, void* pe,
                      void* z1, float* pn, void* h1, void* pe_pre, int32_t gelu, int32_t dtype, segger_stream_t stream);
size_t segger_posmlp_bwd_workspace_bytes(int64_t n_rows);
int segger_posmlp_bwd(const void* g, int64_t ld_g, const void* z1, const float* pn, const void* w2_t, int64_t n_rows,
                      float max_period, int32_t dtype, float* grad_w0, float* grad_b0, float* grad_w2, float* grad_b2,
                      void* workspace, size_t workspace_bytes, segger_stream_t stream);
size_t segger_posmlp_bwd_pair_workspace_bytes(int64_t n_rows_a, int64_t n_rows_b);
int segger_posmlp_bwd_pair(const void* g_a, int64_t ld_ga, const void* z1_a, const float* pn_a, int64_t n_rows_a,
                           const void* g_b, int64_t ld_gb, const void* z1_b, const float* pn_b, int64_t n_rows_b,
                           const void* w2_t, float max_period, int32_t dtype, float* grad_w0, float* grad_b0,
                           float* grad_w2, float* grad_b2, void* workspace, size_t workspace_bytes,
                           segger_stream_t stream);
int segger_posmlp_wgrad(const void* dz1, int64_t ld_dz1, const float* pn, int64_t n_rows, float max_period,
                        int32_t dtype, float* grad_w0, float* grad_b0, void* workspace, size_t workspace_bytes,
                        segger_stream_t stream);
int segger_embed_gelu_fwd(const float* table, const int32_t* ids, const void* pe, int64_t ld_pe, int64_t n,
                          int32_t n_rows_table, int32_t D, void* out, int64_t ld_out, int32_t dtype,
                          segger_stream_t stream);
size_t segger_embed_gelu_bwd_workspace_bytes(int64_t n, int32_t n_rows_table, int32_t D);
int segger_embed_gelu_bwd(const void* gx0, int64_t ld_g, const float* table, const void* pe, int64_t ld_pe,
                          int64_t n, int32_t n_rows_table, int32_t D, void* gpe, int64_t ld_gpe, float* gtable,
                          const int64_t* gene_ptr, const int32_t* gene_rows, void* workspace, size_t workspace_bytes,
                          int32_t dtype, segger_stream_t stream);
/* segger_front_join_fwd/bwd: the encoder's layer-0 input of BOTH node types, one launch each way
 * (ist_encoder.py:312-320: x = {k: gelu(cat(lin_first[k](x[k]), pos_emb(pos[k])))}):
 *   out_tx[r] = gelu(cat(table[ids[r]], pe[r]))  r < n_tx;   out_bd[r] = gelu(cat(xb[r], pe[n_tx + r]))  r < n_bd
 * with `pe` the positional embeddings of the two types back to back ([n_tx + n_bd, D]: one embedder call) and xb =
 * lin_first['bd'](x_bd).  bwd: g_pe [n_tx + n_bd, D] = g[:, D:] * gelu'(pe) written as ONE matrix, g_xb = g_bd[:, :D] *
 * gelu'(xb), g_table (optional) as segger_embed_gelu_bwd (gene_ptr / gene_rows / workspace of
 * segger_embed_gelu_bwd_workspace_bytes(n_tx, n_rows_table, D)).  It replaces torch's cat + GELU (+ their backward, and
 * the full-size cat that joins the two slices' gradients) on the boundary side of a small batch. */
typedef struct segger_front_join_args {
  const float* table; const int32_t* ids; int32_t n_rows_table; int32_t D; int32_t dtype; int32_t reserved_;
  const void* pe; int64_t ld_pe; int64_t n_tx, n_bd;
  const void* xb; int64_t ld_xb;
  void* out_tx; int64_t ld_out_tx; void* out_bd; int64_t ld_out_bd;                      /* forward outputs [n, 2D] */
  const void* g_tx; int64_t ld_g_tx; const void* g_bd; int64_t ld_g_bd;                  /* backward inputs [n, 2D] */
  void* g_pe; int64_t ld_g_pe; void* g_xb; int64_t ld_g_xb;                              /* backward outputs */
  float* g_table; const int64_t* gene_ptr; const int32_t* gene_rows; void* workspace; size_t workspace_bytes;
} segger_front_join_args;
int segger_front_join_fwd(const segger_front_join_args* args, segger_stream_t stream);
int segger_front_join_bwd(const segger_front_join_args* args, segger_stream_t stream);
int segger_l2norm_fwd(const void* y, int64_t ld_y, int64_t n, int32_t channels, float eps, void* z, int64_t ld_z,
                      int32_t dtype, segger_stream_t stream);
int segger_l2norm_bwd(const void* y, int64_t ld_y, const void* gz, int64_t ld_gz, int64_t n, int32_t channels,
                      float eps, void* gy, int64_t ld_gy, int32_t dtype, segger_stream_t stream);
/* segger_l2norm_many: up to 4 row normalisations in ONE launch (both node types of the encoder's tail, ist_encoder.py:331-332;
 * the boundary side's backward from the loss head's fp32 gradient).  Per segment: gz == NULL -> out = y / max(|y|, eps);
 * otherwise out = d / d y from the incoming gradient gz ([n, C] in the embeddings' dtype, or fp32 when gz_f32 != 0). */
typedef struct segger_l2norm_seg {
  const void* y; int64_t ld_y; int64_t n;
  void* out; int64_t ld_out;
  const void* gz; int64_t ld_gz; int32_t gz_f32; int32_t reserved_;
} segger_l2norm_seg;
int segger_l2norm_many(const segger_l2norm_seg* segs, int32_t n_segs, int32_t channels, float eps, int32_t dtype,
                       segger_stream_t stream);
/* the same with the incoming gradient given as the sum of two matrices gz + gz2 (gz2 may be NULL): the loss head hands
 * the anchors' stored rows and the atomically accumulated rows over separately (segger_triplet_args.grad_a_rows) */
int segger_l2norm_bwd2(const void* y, int64_t ld_y, const void* gz, int64_t ld_gz, const void* gz2, int64_t ld_gz2, int64_t n,
                       int32_t channels, float eps, void* gy, int64_t ld_gy, int32_t dtype, segger_stream_t stream);
/* out[s, :] = sum of the rows x[seg_rows[seg_ptr[s] : seg_ptr[s+1]], :] in fp32 (deterministic, no atomics): the
 * scatter-add of per-edge rows into a small table, e.g. the boundary-side gradient of the triplet loss
 * (lightning_model.py:182-187 autograd).  seg_ptr / seg_rows = indptr / col of segger_csr_from_coo(row = segment id of
 * every x row, col = 0..n-1).  D % 8 == 0, D <= 2048. */
size_t segger_segment_rowsum_workspace_bytes(int64_t n, int32_t n_segments, int32_t D);
int segger_segment_rowsum(const void* x, int64_t ld, int64_t n, int32_t D, int32_t dtype, const int64_t* seg_ptr,
                          const int32_t* seg_rows, int32_t n_segments, float* out, void* workspace,
                          size_t workspace_bytes, segger_stream_t stream);
size_t segger_colsum_workspace_bytes(int64_t n, int32_t cols);
int segger_colsum(const void* x, int64_t ld, int64_t n, int32_t cols, int32_t dtype, float* out,
                  void* workspace, size_t workspace_bytes, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Exact 2-D k-nearest neighbours on a uniform grid: the step BEFORE the hot path
 * (graph construction).  Replaces scipy.spatial.KDTree(points).query(queries, k,
 * distance_upper_bound=max_dist, workers=-1) in src/segger/data/utils/neighbors.py:122-163.
 *   points [n,2] fp32; queries [m,2] fp32 or NULL (= points, then m must equal n);
 *   grid: origin (x0,y0), square cells of side `cell`, nx x ny cells (points outside are
 *   clamped into the border cells, so any grid is valid; the host picks ~2 points per cell);
 *   nbr [m,k] int32: neighbour ids sorted by distance, padded with n (scipy's convention);
 *   dist [m,k] fp32 or NULL: distances, +inf for padding;  1 <= k <= 64; max_dist may be +inf and is a
 *   strict bound, as scipy's is: a point at exactly max_dist (squared fp32 distances compared) is padding.
 * ---------------------------------------------------------------------- */
size_t segger_knn_workspace_bytes(int64_t n_points, int32_t nx, int32_t ny);
int segger_knn_grid(const float* points, int64_t n_points, const float* queries, int64_t n_queries, int32_t k,
                    float max_dist, float x0, float y0, float cell, int32_t nx, int32_t ny,
                    int32_t* nbr, float* dist, void* workspace, size_t workspace_bytes, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Adaptive quadtree tiling of a slide: the step that decides what a tile is (the reference's default,
 * tiling_mode="adaptive").  Replaces cuspatial.quadtree_on_points + the retry loop around its invalid trees in
 * src/segger/geometry/quadtree.py:142-216 (get_quadtree_index), the key decoding at :56-94, and -- for point
 * geometries -- the `intersects` join + drop_duplicates of QuadTreeTiling / Tiling.label in
 * src/segger/data/tiling.py:152-196,198-233.
 *
 * Frame (the host computes it in float64, quadtree.py:33-42): origin (x0, y0), square cells of side `cell` (a power
 * of two >= 1), 2^depth x 2^depth of them, 1 <= depth <= 15.  Cell of a point: ix = clamp(floor((double(x) - x0) / cell),
 * 0, 2^depth - 1), iy alike; Morton key = two bits per level, x in the even bit, y in the odd bit (< 2^30).
 * The node at depth d in 1..depth is the prefix key >> 2 (depth - d); the root is never a leaf.  A node with c > 0
 * points is a leaf iff every proper ancestor holds more than max_size points and (c <= max_size or d == depth); empty
 * quadrants are no leaves.  Leaves are numbered in ascending (d, prefix) order.
 *
 * segger_quadtree_build: points [n,2] fp32 (8-byte aligned), 1 <= n < 2^31.  Outputs, all caller-allocated:
 *   leaf_key / leaf_depth / leaf_count [leaf_cap] int32: prefix, depth d and population of leaf i (entries from *n_leaf
 *     on are padding: -1 / 0 / 0);
 *   morton_lo / morton_id [leaf_cap] int32: the same leaves sorted by the first key of their range,
 *     prefix << 2 (depth - d), with the leaf id (padding: -1 / -1) -- the table segger_quadtree_label searches;
 *   n_leaf [1] int32: the number of leaves (read it back once per slide);
 *   labels [n] int32: the leaf of every build point (always >= 0).
 * Leaf capacity: the nodes split at one depth are disjoint and hold more than max_size points each, and a split turns
 * one node into at most four, so there are at most min(n, 4 + 3 (depth - 1) floor(n / (max_size + 1))) leaves.  Allocate
 * that; the kernels never write past leaf_cap, and *n_leaf > leaf_cap tells that the table is incomplete.
 *
 * segger_quadtree_label: label of arbitrary points against a built tree; -1 outside the closed root box
 * [x0, x1] x [y0, y1] and inside empty quadrants.  Half-open by construction: a point on a shared border belongs to the
 * upper cell (the reference's join gives it to whichever tile comes first in an unspecified order).
 *
 * segger_quadtree_workspace_bytes: bytes of workspace for a build (two key arrays, the radix sort's storage, the work
 * lists), or a negative SEGGER_E* code for arguments a build would reject.
 * ---------------------------------------------------------------------- */
int64_t segger_quadtree_workspace_bytes(int64_t n_points, int32_t depth, int64_t max_size, int64_t leaf_cap);
int segger_quadtree_build(const float* points, int64_t n_points, double x0, double y0, double cell, int32_t depth,
                          int64_t max_size, int64_t leaf_cap, int32_t* leaf_key, int32_t* leaf_depth, int32_t* leaf_count,
                          int32_t* morton_lo, int32_t* morton_id, int32_t* n_leaf, int32_t* labels, void* workspace,
                          size_t workspace_bytes, segger_stream_t stream);
int segger_quadtree_label(const float* points, int64_t n_points, double x0, double y0, double x1, double y1, double cell,
                          int32_t depth, const int32_t* leaf_key, const int32_t* leaf_depth, const int32_t* morton_lo,
                          const int32_t* morton_id, int64_t n_leaf, int32_t* labels, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Streaming transcript -> cell assignment: the best row per transcript over the prediction batches of a slide, kept
 * on the device batch by batch.  Replaces the concat + sort + unique of ISTSegmentationWriter.assign_transcripts_to_cells
 * (src/segger/data/writer.py:186-190), which needs every prediction row of the slide at once.
 *
 * State, caller-allocated and sized by n_tx, the number of transcripts of the slide (the row_index domain,
 * 1 <= n_tx < 2^31); the caller zeroes best_key and counters before the first update:
 *   best_key [n_tx] uint64, 0 = "not seen";  cell [n_tx] int32;  gene_out [n_tx] int32;
 *   counters [2] uint64: rows seen so far (the base sequence number), rows dropped.
 *
 * Key of a candidate row with similarity s and sequence number q (its position in the concatenation of everything fed
 * so far, q < 2^32):
 *   b   = bits(s + 0.0f)                      -0.0 becomes +0.0 (denormals are kept)
 *   b   = isnan(s) ? 0x7FC00000 : b           one canonical NaN, above +inf like torch.sort
 *   ord = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000)
 *   key = ((uint64)ord << 32) | (0xFFFFFFFF - q)
 * A larger key is a higher similarity and, at equal similarity, the earlier row: the rule of the stable sorts it
 * replaces.  key == 0 cannot occur for a real row.
 *
 * segger_assign_update: tx_index [n] int64, seg [n] int64, sim [n] fp32, gene [n] int32, mask [n] uint8 or NULL
 * (0 = skip the row).  Enqueues three steps in stream order and never waits for the device:
 *   1. per row: skipped if masked out; if tx_index is outside [0, n_tx) or q = counters[0] + i does not fit 32 bits the
 *      row is counted in counters[1] and skipped -- nothing is ever written out of range; otherwise
 *      atomicMax(best_key[tx], key);
 *   2. per row whose key equals best_key[tx]: cell[tx] = (int32)seg, gene_out[tx] = gene.  Sequence numbers are
 *      unique, so exactly one row per transcript wins and nothing races;
 *   3. counters[0] += n, in a launch of its own, so no block of steps 1-2 sees it early.
 * The result does not depend on the order or the batching of the rows, bit for bit.  The base sequence number lives in
 * device memory: a call captured in a hipGraph stays correct on replay.  n == 0 launches nothing.  Cell encodings
 * must fit int32.
 *
 * segger_assign_finalize: similarity_out [n_tx] fp32 = the winning similarity (ord inverted; 0 where not seen),
 * seen_out [n_tx] uint8 = best_key != 0.
 *
 * Both reject on the host with SEGGER_EINVAL, launching nothing: a NULL pointer (mask excepted), a misaligned pointer,
 * a negative n, n_tx < 1, n_tx >= 2^31.
 * ---------------------------------------------------------------------- */
int segger_assign_update(const int64_t* tx_index, const int64_t* seg, const float* sim, const int32_t* gene,
                         const uint8_t* mask, int64_t n, uint64_t* best_key, int32_t* cell, int32_t* gene_out,
                         uint64_t* counters, int64_t n_tx, segger_stream_t stream);
int segger_assign_finalize(const uint64_t* best_key, int64_t n_tx, float* similarity_out, uint8_t* seen_out,
                           segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Expression matrix of a segmentation: cell x gene counts of the segmented transcripts, in canonical CSR, with the
 * per-pair mean similarity and the per-cell row count and mean position.  Replaces the filter + polars group-by +
 * scipy coo_matrix(...).tocsr() of ISTSegmentationWriter.write_anndata (src/segger/data/writer.py:91-129) and
 * anndata_from_transcripts (src/segger/data/utils/anndata.py:18-102).
 * Purely additive: two new symbols, no existing signature or struct changes, so SEGGER_ABI_VERSION stays 32.
 *
 * Inputs over the n_rows deduplicated transcripts of a slide (0 <= n_rows < 2^31), in ascending row_index:
 *   cell [n_rows] int32 (-1 = unassigned), gene [n_rows] int32, similarity [n_rows] fp32,
 *   threshold [n_rows] fp64 (the similarity_threshold column; NaN = the gene has no threshold),
 *   xy [n_rows, 2] fp32 or NULL;  1 <= n_cells < 2^31, 1 <= n_genes < 2^31 (ids are int32; n_cells * n_genes < 2^63).
 * A row is KEPT iff cell >= 0 && (double)similarity >= threshold: a NaN on either side is not kept, equality is.  A kept
 * row with cell >= n_cells or gene outside [0, n_genes) is never used as an index: it is counted in n_bad and takes no
 * part in any other output.
 *
 * Outputs, caller-allocated at their upper bounds, the real sizes in counters [5] uint64 =
 * {n_kept, nnz, n_cells_present, n_genes_present, n_bad} (n_kept counts the in-range kept rows):
 *   cell_ids [min(n_rows, n_cells)] int32        ascending cells that own a kept row       (n_cells_present entries)
 *   gene_ids [min(n_rows, n_genes)] int32        ascending genes that own a kept row       (n_genes_present entries)
 *   indptr [min(n_rows, n_cells) + 1] int64      CSR row pointers                          (n_cells_present + 1 entries)
 *   indices [n_rows] int32                       POSITION IN gene_ids, strictly ascending inside a row  (nnz entries)
 *   counts [n_rows] int32                        kept rows of the (cell, gene) pair        (nnz entries)
 *   mean_similarity [n_rows] fp64                mean similarity of the pair               (nnz entries)
 *   cell_count [min(n_rows, n_cells)] int64      kept rows of the cell                     (n_cells_present entries)
 *   centroid [min(n_rows, n_cells), 2] fp64      mean xy of the cell; NULL exactly when xy is NULL
 * Entries past the real sizes are not written.
 *
 * Route: key = (cell << bit_length(n_genes - 1)) | gene per kept row, the sentinel n_cells << bit_length(n_genes - 1) for
 * the others; one stable radix sort over bit_length(sentinel) bits with the row position as value; a compaction of the run
 * heads; one lane per run (runs of up to 64 rows, summed first row to last) or one wave per run (longer: lane l sums
 * rows l, l + 64, ... and the 64 partial sums meet in a fixed butterfly); the same reduction over the rows of a cell in
 * sorted order (gene by gene, ascending row position) for cell_count and centroid.
 * Arithmetic: counts and indices are exact; sums are float64; every output is a function of the inputs alone -- the same
 * bits from run to run and for any launch geometry.  No floating-point atomics; integer atomics only count.
 *
 * Workspace: segger_expression_workspace_bytes (28 bytes per row + 8 per cell + 8 per gene + the radix sort's storage),
 * 256-byte aligned; a negative SEGGER_E* code for sizes a build would reject.  n_rows == 0 launches nothing: the
 * caller's zeroed counters and indptr[0] are the result (both must be given; every other pointer is ignored).  Otherwise
 * the build zeroes counters itself, every call.
 * Rejected on the host with SEGGER_EINVAL, nothing launched: a NULL pointer (xy and centroid excepted, as a pair), a
 * misaligned pointer, n_rows < 0 or >= 2^31, n_cells < 1, n_genes < 1, an overflowing n_cells * n_genes; a workspace
 * below segger_expression_workspace_bytes gives SEGGER_EWORKSPACE.
 * ---------------------------------------------------------------------- */
int64_t segger_expression_workspace_bytes(int64_t n_rows, int64_t n_cells, int64_t n_genes);
int segger_expression_build(const int32_t* cell, const int32_t* gene, const float* similarity, const double* threshold,
                            const float* xy, int64_t n_rows, int64_t n_cells, int64_t n_genes, int32_t* cell_ids,
                            int32_t* gene_ids, int64_t* indptr, int32_t* indices, int32_t* counts, double* mean_similarity,
                            int64_t* cell_count, double* centroid, uint64_t* counters, void* workspace,
                            size_t workspace_bytes, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Per-gene similarity thresholds of a segmentation: min(Yen, Li) over the ASSIGNED rows (cell >= 0) of every gene.
 * Replaces the per-gene polars loop of ISTSegmentationWriter.assign_transcripts_to_cells (src/segger/data/writer.py:
 * 196-241) and the sorts / float64 copies of postprocess.per_gene_thresholds.  The reference's 10 M-per-gene
 * subsampling (polars RNG) is not reproduced: every value is used.
 * Purely additive: two new symbols, no existing signature or struct changes, so SEGGER_ABI_VERSION stays 32.
 *
 * Inputs over n_rows rows (0 <= n_rows < 2^31): similarity [n_rows] fp32, gene [n_rows] int32, cell [n_rows] int32
 * (-1 = unassigned); 1 <= n_genes < 2^31 is the gene id domain; max_iter >= 1 (the reference gives up after 250).
 * An assigned row with gene outside [0, n_genes) is counted in n_bad, an assigned in-range row with a NaN similarity in
 * n_nan; neither is used as an index or takes part in any output.
 *
 * Outputs, dense over the gene ids, all [n_genes]: threshold fp64, yen fp64, li fp64, count int64 (assigned rows of
 * the gene), converged uint8; counters [4] int64 = {n_assigned (the rows used), n_genes_present, n_bad, n_nan}, zeroed
 * by the call.  A gene without a row: threshold = yen = li = NaN, count = 0, converged = 1.  Otherwise
 *   yen: 256 bins over [min, max] (a gene of one value: [min - 0.5, max + 0.5]); edges lo + i * (hi - lo) / 256, edge
 *        256 pinned to hi; a value is in bin i iff edge_i <= v < edge_{i+1}, the last bin closed (numpy.histogram);
 *        pmf = counts / count; P1 = cumsum(pmf), P1sq = cumsum(pmf^2), P2sq = cumsum(pmf^2 reversed) reversed, each a
 *        sequential float64 running sum; crit_i = log((1 / (P1sq_i * P2sq_{i+1})) * (P1_i * (1 - P1_i))^2), i < 255;
 *        k = the first NaN of crit, else its first maximum (numpy.argmax); yen = (edge_k + edge_{k+1}) / 2.
 *   li:  on a = v - min in float64: tol = half the smallest positive difference of consecutive sorted a (-0.0 and +0.0
 *        are equal: no gap); t_next = mean(a), t_curr = -2 tol, calls = 1; while |t_next - t_curr| > tol: t_curr = t_next;
 *        mean_back = mean(a <= t_curr), mean_fore = mean(a > t_curr); stop if mean_back == 0; t_next = (mean_back -
 *        mean_fore) / (log mean_back - log mean_fore); if ++calls > max_iter the gene has FAILED (converged = 0) and
 *        stops.  li = t_next + min; a gene of one value: li = min, converged = 1.
 *   threshold = li < yen ? li : yen, also for a failed gene: the median back-fill of writer.py:238-241 is the caller's.
 *
 * Route: key = ((uint64)gene << 32) | ord(similarity) per used row (ord: the order-preserving uint32 image of the
 * float's bits, b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000)), all ones for the others; ONE keys-only radix sort over
 * 32 + bit_length(n_genes) bits -- the sorted keys are the data, there is no value array and no permutation; segment
 * bounds from adjacent high words; float64 sums of a over chunks of SEGGER_THRESHOLDS_CHUNK sorted positions that lie
 * inside one gene (thread t of 256 adds positions t, t + 256, ..., a fixed butterfly per wave, the four waves first to
 * last) and a sequential prefix over a gene's chunks; then one workgroup per gene: Yen's counts are differences of
 * binary-search positions of the 257 edges, a Li iteration is one binary search plus the chunk prefix plus a sum of
 * fewer than SEGGER_THRESHOLDS_CHUNK rows.  Every output is a function of the multiset of used rows: the same bits
 * from run to run and for any order of the rows.  No floating-point atomics; integer atomics count and take the minimum
 * gap (as the bit pattern of a positive double).
 *
 * Workspace: segger_thresholds_workspace_bytes = 16 bytes per row (the keys, in and out of the sort) + the radix sort's
 * own storage (histograms and, on gfx950, one more array of keys: 8 bytes per row) + 16 bytes per gene + 8 bytes per
 * SEGGER_THRESHOLDS_CHUNK rows, each part rounded up to 256 bytes; 256-byte aligned; a negative SEGGER_E* code for
 * sizes a build would reject.  With n_rows and n_genes below 2^31 the sum is below 2^37: it cannot overflow.
 * n_rows == 0 is a no-op that fills the per-gene outputs with the values of a gene without a row and zeroes the counters:
 * similarity, gene, cell and workspace are not looked at and may be NULL.
 * Rejected on the host with SEGGER_EINVAL, nothing launched: n_rows < 0 or >= 2^31, n_genes < 1 or >= 2^31,
 * max_iter < 1, workspace_bytes < 0, a NULL pointer, a misaligned pointer; a workspace below
 * segger_thresholds_workspace_bytes gives SEGGER_EWORKSPACE.
 * ---------------------------------------------------------------------- */
#define SEGGER_THRESHOLDS_CHUNK 1024
int64_t segger_thresholds_workspace_bytes(int64_t n_rows, int64_t n_genes);
int segger_thresholds_build(const float* similarity, const int32_t* gene, const int32_t* cell, int64_t n_rows,
                            int64_t n_genes, int32_t max_iter, double* threshold, double* yen, double* li, int64_t* count,
                            uint8_t* converged, int64_t* counters, void* workspace, int64_t workspace_bytes,
                            segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Boundary and gene features of a count matrix: the two kernels behind segger_amd.features.expression_features, which
 * restates the reference's setup_anndata (src/segger/data/utils/anndata.py:184-259): normalize_total, np.corrcoef of
 * the densified matrix, PCA of the correlation matrix (X_corr), PCA of the cells (X_pca).  Both the correlation and the
 * covariance come from ONE second-moment matrix of the weighted sparse rows; nothing dense of size n_rows x n_cols
 * exists anywhere.  csrc/features.hip.  Purely additive: four new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * The matrix is CSR as segger_expression_build leaves it: indptr [n_rows + 1] int64, indices [nnz] int32 strictly
 * ascending inside a row, values [nnz] int32; row_weight [n_rows] fp64 (finite).  0 <= n_rows < 2^31,
 * 1 <= n_cols <= SEGGER_FEATURES_MAX_COLS, nnz >= 0 (indices and values may be NULL when it is 0).  Row extents are
 * clamped to [0, nnz] and a column outside [0, n_cols) is never used as an index.
 *
 * segger_sparse_gram:  S [n_cols, n_cols] fp64 = sum_r w_r^2 x_r x_r^T,  s [n_cols] fp64 = sum_r w_r x_r.
 *   A row of weight 0 takes no part (this is how a caller restricts the sums to a subset of the rows).  Both triangles
 *   of S are written; S[i, j] and S[j, i] have the same bits (the upper triangle is computed, then mirrored).
 *   Route: one workgroup per pair (ti <= tj) of SEGGER_FEATURES_TILE-column tiles and per slab of rows; 32 rows at a time
 *   are densified into zero-filled LDS tiles (entry * w_r; the start of a tile's range by binary search in the row) and
 *   accumulated with v_mfma_f64_16x16x4_f64; each workgroup leaves one tile of partial sums and a second kernel adds the
 *   slabs first to last.  segger_features_gram_slabs(n_rows, n_cols) = min(ceil(n_rows / SEGGER_FEATURES_SLAB_ROWS),
 *   ceil(SEGGER_FEATURES_TARGET_GROUPS / n_pairs), SEGGER_FEATURES_MAX_SLABS), at least 1, n_pairs = t (t + 1) / 2,
 *   t = ceil(n_cols / SEGGER_FEATURES_TILE); a slab is ceil(n_rows / slabs) rows rounded up to a multiple of 32.  The
 *   slab count and every summation order are functions of (n_rows, n_cols) alone: the same bits from call to call and
 *   on any stream.  No floating-point atomics, no scratch memory.  n_rows == 0 zeroes S and s without a kernel.
 *   Workspace: segger_features_workspace_bytes(n_rows, n_cols) = slabs * (n_pairs * TILE^2 + t * TILE) * 8 bytes,
 *   256-byte aligned: fewer than SEGGER_FEATURES_TARGET_GROUPS + n_pairs tiles of 32 KiB plus the column sums -- it
 *   follows the number of column tiles, never n_rows * n_cols (33 MiB at 10^6 x 500).  Both size queries return a
 *   negative SEGGER_E* code for sizes a call would reject.
 *
 * segger_sparse_project:  out [n_rows, k] = w_r * sum_j x_rj V[j, :] - offset,  V [n_cols, k] fp64 row-major,
 *   offset [k] fp64, 1 <= k <= SEGGER_FEATURES_MAX_K, out fp32 (out_f64 = 0) or fp64 (out_f64 = 1).  One wave per row;
 *   lane l owns columns l, l + 64, l + 128, l + 192 and adds the row's entries in CSR order with float64 FMAs, then
 *   rounds fma(w_r, sum, -offset) once to the output type: bit-reproducible.  w_r == 0 gives exactly -offset.
 *
 * Rejected on the host with SEGGER_EINVAL, nothing launched: a NULL or misaligned pointer, n_rows < 0 or >= 2^31,
 * n_cols < 1 or > SEGGER_FEATURES_MAX_COLS, nnz < 0, k outside 1 .. SEGGER_FEATURES_MAX_K, out_f64 other than 0 / 1,
 * workspace_bytes < 0; a workspace below segger_features_workspace_bytes gives SEGGER_EWORKSPACE.
 * ---------------------------------------------------------------------- */
#define SEGGER_FEATURES_TILE 64
#define SEGGER_FEATURES_SLAB_ROWS 512
#define SEGGER_FEATURES_MAX_SLABS 32
#define SEGGER_FEATURES_TARGET_GROUPS 1024
#define SEGGER_FEATURES_MAX_COLS 32768
#define SEGGER_FEATURES_MAX_K 256
int64_t segger_features_gram_slabs(int64_t n_rows, int64_t n_cols);
int64_t segger_features_workspace_bytes(int64_t n_rows, int64_t n_cols);
int segger_sparse_gram(const int64_t* indptr, const int32_t* indices, const int32_t* values, const double* row_weight,
                       int64_t n_rows, int64_t n_cols, int64_t nnz, double* S, double* s, void* workspace,
                       int64_t workspace_bytes, segger_stream_t stream);
int segger_sparse_project(const int64_t* indptr, const int32_t* indices, const int32_t* values, const double* row_weight,
                          int64_t n_rows, int64_t n_cols, int64_t nnz, const double* V, const double* offset, int32_t k,
                          void* out, int32_t out_f64, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Phenograph clustering: the kernels behind segger_amd.phenograph (knn_bruteforce, jaccard_graph, louvain), which
 * restates the reference's phenograph_rapids (src/segger/data/utils/neighbors.py:18-51: cuML kneighbors, cuGraph jaccard,
 * cuGraph louvain) without RAPIDS.  csrc/phenograph.hip.  Purely additive: six new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * segger_knn_bruteforce:  for every row of X [n, d] fp32 row-major its k nearest rows of X, ITSELF INCLUDED, as
 *   idx [n, k] int32 and dist2 [n, k] fp32 (squared Euclidean), each row sorted by (dist2, idx).  1 <= n < 2^31,
 *   1 <= d <= SEGGER_KNN_BF_MAX_D, 1 <= k <= min(SEGGER_KNN_BF_MAX_K, n); n * k may pass 2^31 (64-bit offsets).
 *   Selection runs on the score (|a|^2 + |b|^2) - 2 a.b: the norms are fp32 FMA chains over ascending dimensions, the
 *   inner products v_mfma_f32_16x16x4_f32 (an fp32 FMA chain in a fixed permutation of the dimensions, d padded with
 *   zeros to 32 / 64 / 128 / 256), the score fmaf(-2, a.b, |a|^2 + |b|^2).  A workgroup of 512 threads owns 128 query
 *   rows, resident in registers, against one slab of candidate rows staged 64 at a time through LDS; every query row
 *   keeps its k smallest (score bits in float order, index) keys in the lanes of the wave that owns it and merges a tile
 *   only when one of its 64 candidates beats the k-th (bitonic sort + merge in the wave).  The kept set is the k
 *   smallest keys of the slab whatever the order of arrival.  segger_knn_bruteforce_slabs(n, d, k) = min(ceil(
 *   SEGGER_KNN_BF_TARGET_GROUPS / ceil(n / 128)), floor(n / 128), SEGGER_KNN_BF_MAX_SLABS), at least 1; a slab is
 *   ceil(n / slabs) rows rounded up to a multiple of 64, and the count returned is ceil(n / that).  The finish kernel
 *   (one wave per row) merges the slabs' lists, recomputes the k distances as acc = fmaf(a_t - b_t, a_t - b_t, acc) over
 *   t ascending and sorts.  No n x n or n x tile score matrix is written; no floating-point atomics; no scratch; no loop
 *   bound depends on the data: the same bits from call to call and on any stream.  Rows that hold NaN are not supported.
 *   Workspace: segger_knn_bruteforce_workspace_bytes(n, d, k) = n * 4 rounded up to 256, plus slabs * n * k * 8 bytes.
 *
 * segger_jaccard_weights:  weight [nnz] fp64 of every stored edge of a simple undirected graph in CSR (indptr [n + 1]
 *   int64, indices [nnz] int32 ascending inside a row, both directions stored, no self-loops): |N[u] & N[v]| /
 *   |N[u] | N[v]| over the CLOSED neighbourhoods N[x] = adj[x] + {x}.  One thread per edge finds its row by binary search
 *   in indptr and merges the two adjacency lists (any degree); the weight is ONE fp64 division of the two integers, so
 *   weight[u -> v] and weight[v -> u] have the same bits.
 *
 * segger_louvain_move:  one sub-round of synchronous local moving.  weight [nnz] and kdeg [n] (the weighted degree, self
 *   weight included) are int64 fixed point (round(w * 2^32)); comm [n] int32, tot [n] int64 and size [n] int32 are the
 *   community of every vertex and the degree sum and member count of every community.  For every vertex v with
 *   v mod n_sub == sub, one wave evaluates g(c) = k_vc - (gamma * k_v) * tot_c / two_m in fp64 for the community c of
 *   every neighbour (k_vc an exact integer sum; for v's own community tot excludes k_v), proposes the largest g, the
 *   lowest c on a tie, only if it is strictly above staying, and never from a singleton into a singleton of a higher id;
 *   all reads are of the state at entry.  A second kernel applies the proposals with integer atomics (exact in any
 *   order).  The neighbour sums are quadratic in the degree inside the wave: correct for any degree, no fixed-size list.
 *
 * segger_louvain_modularity:  in_c [n] int64 = self_weight of the members + the stored edges inside the community
 *   (integer atomics), then q[0] = sum_c in_c / two_m - (gamma * (tot_c / two_m)) * (tot_c / two_m) in fp64 by ONE
 *   workgroup: thread t adds the terms t, t + 256, ... in turn, the 256 sums fold in halves.  A fixed order.
 *
 * Rejected on the host with SEGGER_EINVAL, nothing launched: a NULL or misaligned pointer, n, d or k out of range,
 * k > n, nnz < 0, sub / n_sub out of range, two_m <= 0, gamma < 0, workspace_bytes < 0; a workspace below
 * segger_knn_bruteforce_workspace_bytes gives SEGGER_EWORKSPACE.  The two size queries return the negative code.
 * ---------------------------------------------------------------------- */
#define SEGGER_KNN_BF_MAX_D 256
#define SEGGER_KNN_BF_MAX_K 64
#define SEGGER_KNN_BF_TARGET_GROUPS 512
#define SEGGER_KNN_BF_MAX_SLABS 32
#define SEGGER_LOUVAIN_MAX_SUBROUNDS 64
int64_t segger_knn_bruteforce_slabs(int64_t n, int32_t d, int32_t k);
int64_t segger_knn_bruteforce_workspace_bytes(int64_t n, int32_t d, int32_t k);
int segger_knn_bruteforce(const float* X, int64_t n, int32_t d, int32_t k, int32_t* idx, float* dist2, void* workspace,
                          int64_t workspace_bytes, segger_stream_t stream);
int segger_jaccard_weights(const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz, double* weight,
                           segger_stream_t stream);
int segger_louvain_move(const int64_t* indptr, const int32_t* indices, const int64_t* weight, const int64_t* kdeg, int64_t n,
                        int64_t nnz, int32_t sub, int32_t n_sub, double gamma, double two_m, int32_t* comm, int64_t* tot,
                        int32_t* size, int32_t* proposal, segger_stream_t stream);
int segger_louvain_modularity(const int64_t* indptr, const int32_t* indices, const int64_t* weight, const int64_t* self_weight,
                              const int32_t* comm, const int64_t* tot, int64_t n, int64_t nnz, double gamma, double two_m,
                              int64_t* in_c, double* q, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Contamination scoring of a segmentation: the kernels behind segger_amd.validation (neighbor_frequencies,
 * calculate_contamination), which restates the reference's src/segger/validation/contamination.py without cuML, scanpy or
 * AnnData.  csrc/contamination.hip.  Purely additive: two new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * segger_neighbor_frequencies:  nbr [n, k] int32 and dist [n, k] fp32 are the tables segger_knn_grid returns for a point
 *   set queried against itself (the point itself included at distance 0, the padding id n), labels [n] int32 the type of
 *   every point.  A neighbour counts iff its id is in [0, n), (double) dist <= max_distance (+inf: no limit) and its label
 *   is in [0, n_types) -- -1, or any other value outside the range, is "unlabelled" and is never used as an index.
 *   counts [n, n_types] int32 = the neighbours of every type; freq [n, n_types] fp32 = (float)(count * (1.0 / sum)) with
 *   the product in fp64, all zero when sum = 0.  1 <= k <= SEGGER_CONTAM_MAX_K, 1 <= n_types <= SEGGER_CONTAM_MAX_TYPES.
 *   One wave per point, every output element written once by the lane that owns it: no atomics.
 *
 * segger_contamination_posterior:  for every stored entry (row r, column c, count v) of a CSR count matrix (indptr
 *   [n_rows + 1] int64, indices [nnz] int32, counts [nnz] int32) a three-way posterior against a per-type expression table.
 *   gene_map [n_cols] int32 gives the table column g of CSR column c (outside [0, n_ref_genes): the table lacks the gene),
 *   host_type [n_rows] int32 the row's type (outside [0, n_types): none), freq [n_rows, n_types] fp32 the neighbour
 *   frequencies.  THE TABLE IS GENE-MAJOR: Lt [n_ref_genes, ld_L] fp32 with Lt[g, t] = L[t, g], 16-byte aligned, ld_L a
 *   multiple of 4 and >= n_types (columns n_types .. ld_L - 1 are never read); back [n_ref_genes] fp64 is the background
 *   A @ L.  In fp64, the types summed in ascending order:
 *     P_self  = Lt[g, type_r], or eps when the row has no type;
 *     P_neigh = sum_{t != type_r} freq[r, t] * Lt[g, t] + eps  (all t when the row has no type);
 *     P_back  = back[g] + eps;
 *     q_x     = alpha_x * P_x / ((alpha_self * P_self + alpha_neighbor * P_neigh) + alpha_background * P_back).
 *   q_self, q_neighbor, q_background [nnz] fp32 are each rounded once from fp64; contamination [nnz] int32 = v where the fp64
 *   q_self < contam_cutoff, else 0; an entry whose gene the table lacks gets three zeros and is never flagged.  Per row:
 *   contaminated and total int64 (exact sums of the flagged and of all counts) and percent fp64 = (100.0 * contaminated) /
 *   max(total, 1).  One wave per row: the row's frequencies are staged in LDS with the host type's slot zeroed, lanes take
 *   the entries 64 at a time and read four types of Lt per load; the table itself is copied into LDS (row stride padded
 *   so that stride / 4 is odd) when n_ref_genes * stride * 4 plus the four strips fit SEGGER_CONTAM_LDS_BYTES (as many
 *   workgroups per CU as its LDS holds copies, at most 8) and is read through L2 otherwise -- the same arithmetic in the same order on both routes.  Nothing of size nnz x n_types exists;
 *   no atomics; the same bits from call to call.
 *
 * Rejected on the host with SEGGER_EINVAL, nothing launched: a NULL or misaligned pointer, a negative size, 2^31 - 1 rows,
 * points or columns or more, n_types outside 1 .. SEGGER_CONTAM_MAX_TYPES, k outside 1 .. SEGGER_CONTAM_MAX_K, n_ref_genes
 * outside 1 .. SEGGER_CONTAM_MAX_REF_GENES, a bad ld_L, max_distance < 0 or NaN, a non-finite alpha or eps, a NaN cutoff.
 * n = 0 (frequencies), n_rows = 0 or nnz = 0 (posterior) return SEGGER_OK and launch and write nothing: with nnz = 0 the
 * caller zero-fills the three per-row outputs.
 * ---------------------------------------------------------------------- */
#define SEGGER_CONTAM_MAX_TYPES 256
#define SEGGER_CONTAM_MAX_K 64                /* segger_knn_grid's range */
#define SEGGER_CONTAM_MAX_REF_GENES 32768     /* SEGGER_FEATURES_MAX_COLS: the flow table goes through segger_sparse_project */
#define SEGGER_CONTAM_LDS_BYTES 65536
int segger_neighbor_frequencies(const int32_t* nbr, const float* dist, const int32_t* labels, int64_t n, int32_t k,
                                int32_t n_types, double max_distance, int32_t* counts, float* freq, segger_stream_t stream);
int segger_contamination_posterior(const int64_t* indptr, const int32_t* indices, const int32_t* counts, int64_t n_rows,
                                   int64_t n_cols, int64_t nnz, const int32_t* gene_map, const int32_t* host_type,
                                   const float* freq, const float* Lt, int64_t ld_L, const double* back, int32_t n_types,
                                   int32_t n_ref_genes, double alpha_self, double alpha_neighbor, double alpha_background,
                                   double eps, double contam_cutoff, float* q_self, float* q_neighbor, float* q_background,
                                   int32_t* contamination, int64_t* contaminated, int64_t* total, double* percent,
                                   segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Boundary morphology: the parts of the reference's get_polygon_props (src/segger/geometry/morphology.py, stacked into
 * X_morphology at data/utils/anndata.py:296-311) for every polygon of a CSR of rings, without geopandas / shapely.  The
 * kernels behind segger_amd.morphology.  csrc/morphology.hip.  Purely additive: two new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * Input:  ring_offsets [n_polygons + 1] int64 and xy [n_vertices, 2] fp64 (16-byte aligned): polygon p is the single
 *   exterior ring xy[ring_offsets[p] .. ring_offsets[p + 1]), either orientation; no holes, no multi-part polygons.  A ring
 *   whose last vertex equals its first bit for bit is closed and the duplicate is ignored: n below counts the vertices
 *   without it.  Repeated consecutive vertices and vertices collinear with an edge are allowed.
 *
 * Output:  props [n_polygons, SEGGER_MORPH_COLS] fp64, the columns
 *     0 area           |shoelace| / 2                      6 cy
 *     1 hull_area      area of the convex hull H           7 xmin      the bounds, on the coordinates as given (exact)
 *     2 rect_area      minimum-area enclosing rectangle    8 ymin
 *     3 envelope_area  (xmax - xmin) (ymax - ymin)         9 xmax
 *     4 radius         smallest enclosing circle          10 ymax
 *     5 cx             area-weighted centroid             11 n_hull    vertices of H, as fp64
 *   The reference's four columns are area, hull_area / area, rect_area / envelope_area, area / radius^2: the divisions
 *   are the caller's (IEEE: x / 0 = +-inf, 0 / 0 = NaN; nothing is clamped).
 *
 * Arithmetic:  fp64 on coordinates translated to the ring's first vertex (slide coordinates are 10^4 .. 10^5, a cell is
 *   ~10 across: untranslated shoelace terms cancel), FMA contraction off.  One wave owns one polygon: n <= 64 keeps one
 *   vertex per lane in registers; 64 < n <= SEGGER_MORPH_MAX_VERTS stages the ring in LDS.  The polygons are binned by
 *   route on the device (two index lists in the workspace, one integer atomic per wave and route); no floating-point
 *   atomics; every sum is a per-lane sum over ascending vertices followed by a fixed butterfly: a polygon's row has the
 *   same bits from call to call, in whatever batch and at whatever position it is computed.
 *   Hull: gift wrapping from the lowest (x, then y, then index) vertex, counter-clockwise; the next vertex is the most
 *   clockwise one as seen from the current vertex, ties (collinear with it) go to the larger distance, then to the lower
 *   index, and a vertex that coincides with the current one never competes: collinear and duplicate vertices are never
 *   hull vertices, and the march ends at its start after n_hull <= n steps.
 *   Rectangle: the minimum over the hull's edges e of (max_u - min_u) (max_v - min_v) / |e|^2, u and v the projections of
 *   the hull vertices on e and on its normal; the lowest edge index wins a tie.
 *   Circle: exact -- Welzl's iteration over the hull vertices in hull order (no shuffle), support sets of 1, 2 or 3
 *   vertices, the circumcentre computed relative to the first support vertex, r^2 the largest squared distance from the
 *   centre to a support vertex; a vertex is outside iff d^2 > r^2 (1 + SEGGER_MORPH_CIRCLE_SLACK), so a support vertex
 *   never tests as outside its own circle.
 *   Centroid: first vertex + (sum (x_i + x_j) c_ij, sum (y_i + y_j) c_ij) / (3 sum c_ij), c_ij the shoelace terms; the
 *   mean of the vertices when the area is 0.
 *
 * Degenerate rings are results: n = 0 gives a row of NaN; n = 1, 2, or all vertices collinear or identical give
 *   area = hull_area = rect_area = 0, radius = half the extent, n_hull = 1 or 2.
 *
 * Errors found on the device, without a synchronisation: a ring with ring_offsets[p] < 0, ring_offsets[p + 1] <
 *   ring_offsets[p] or ring_offsets[p + 1] > n_vertices gets a row of NaN and sets SEGGER_MORPH_ERR_OFFSETS in the error
 *   word; a ring of more than SEGGER_MORPH_MAX_VERTS vertices gets a row of NaN and SEGGER_MORPH_ERR_CAP (nothing is read
 *   or written out of bounds for either).  The error word is the int32 at byte 0 of the workspace (0 = none), valid once the
 *   stream has run; int32 words 1 and 2 are the polygons that took the register and the LDS route.
 *   The ring lengths live in device memory, so this entry point cannot see the cap without a synchronisation: the cap is
 *   refused BEFORE the call, by the Python wrapper (segger_amd.morphology.polygon_props raises ValueError naming the first
 *   such polygon and launches nothing); a C caller that skips that check gets the NaN row and SEGGER_MORPH_ERR_CAP.
 *
 * Workspace: 256 bytes + 2 x (4 n_polygons rounded up to 256) bytes, 256-byte aligned.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative n_polygons, n_vertices or
 * workspace_bytes, 2^31 - 1 polygons or more, and for n_polygons > 0 a NULL pointer (xy may be NULL when n_vertices = 0), a
 * misaligned pointer, a workspace below segger_morphology_workspace_bytes (which itself returns the negative code for a
 * count out of range).  n_polygons = 0 returns SEGGER_OK without touching a pointer or the device.
 * ---------------------------------------------------------------------- */
#define SEGGER_MORPH_MAX_VERTS 4096           /* 64 KB of fp64 pairs in LDS */
#define SEGGER_MORPH_COLS 12
#define SEGGER_MORPH_CIRCLE_SLACK 0x1p-44     /* relative, on squared distances */
#define SEGGER_MORPH_ERR_OFFSETS 1
#define SEGGER_MORPH_ERR_CAP 2
int64_t segger_morphology_workspace_bytes(int64_t n_polygons);
int segger_polygon_props(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                         double* props /* [P, 12] */, void* workspace, int64_t workspace_bytes, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Points in buffered polygons: every (point, polygon) pair for which the point lies in the polygon grown by a distance
 * d >= 0 of its own -- the reference's points_in_polygons (src/segger/geometry/query.py, a cuSpatial quadtree join) over
 * polygons.buffer(d), which builds the ("tx", "neighbors", "bd") prediction graph of the default mode
 * (src/segger/data/utils/neighbors.py:223-238).  The kernels behind segger_amd.geometry.  csrc/polygon_join.hip.  Purely
 * additive: three new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * The predicate.  For a point t, a ring P (as segger_polygon_props takes it: a CSR of single exterior rings in fp64, either
 *   orientation, a closing duplicate of the first vertex dropped) and a distance d >= 0:
 *     parity(t, P)  the crossing-number test with the half-open rule: an edge (a, b) counts when a.y <= t.y < b.y or
 *                   b.y <= t.y < a.y, and the crossing lies strictly to the right of t;
 *     dist2(t, P)   the smallest squared distance from t to a closed edge segment of the ring;
 *     SEGGER_PJOIN_CONTAINS    dist2 < d d || (parity && dist2 > 0)   the open set: a point on the ring itself is out when
 *                              d == 0 and in when d > 0;
 *     SEGGER_PJOIN_INTERSECTS  dist2 <= d d || parity                 the closed set (what the reference's
 *                              ISTPreprocessor.assign_transcripts_to_boundaries uses through sjoin).
 *   A ring with fewer than 3 vertices (after the closing duplicate is dropped) matches nothing under either predicate.
 *   This is the EXACT offset of the polygon, its Minkowski sum with a disc of radius d.  GEOS, through which the
 *   reference's buffer() goes, replaces each round corner by a polyline (geopandas: 16 segments per quarter circle), so
 *   the two sets differ in slivers at convex corners, at most d (1 - cos(pi / 64)) ~ 0.0012 d wide.  UNVERIFIED: neither
 *   shapely nor GEOS was available where this was written; the arc vertices of GEOS are not reproduced.
 *
 * Arithmetic:  fp64 throughout, the point and the vertices translated to the ring's first vertex before any product (slide
 *   coordinates are 10^4 .. 10^5, a cell is ~10 across), FMA contraction off.  Per edge (a, b):  e = b - a, w = t - a,
 *   cr = e.x w.y - e.y w.x, dot = w.x e.x + w.y e.y, len2 = e.x e.x + e.y e.y;  the edge counts for the parity when
 *   (a.y <= t.y && !(b.y <= t.y) && cr > 0) or (!(a.y <= t.y) && b.y <= t.y && cr < 0);  its squared distance is |w|^2 when
 *   dot <= 0 or len2 == 0, |t - b|^2 when dot >= len2, and cr cr / len2 otherwise;  dist2 is the minimum over the edges.
 *   With coordinates that are exact after the translation, cr is exact: the parity and "on the ring" (dist2 == 0) are.
 *
 * The points are binned into a uniform grid the caller describes (origin x0, y0, cell side, nx x ny cells; points outside
 *   are clamped into the border cells) by a stable keys sort (key = cell << 32 | point id); the kernels read a cell-ordered
 *   fp64 copy of the coordinates and the ids.  One wave owns one polygon: n <= 64 keeps one vertex per lane and broadcasts
 *   the edges across the wave; 64 < n <= SEGGER_MORPH_MAX_VERTS stages the ring in LDS; the polygons are binned by route on
 *   the device (one integer atomic per wave and route).  The wave walks the cells that overlap the ring's bounds grown by
 *   d (1 + 2^-20) + 2^-40 max|bound| (the margin covers the rounding; the cell range is clamped to the grid), 64 points at a
 *   time.  The grid decides the speed and nothing else: the pairs are the same for every grid.
 *
 * Two calls:
 *   segger_polygon_join_count  bins the points, counts the matches of every polygon and scans the counts on the device:
 *       pair_offsets [n_polygons + 1] int64, pair_offsets[p + 1] - pair_offsets[p] = the matches of polygon p and
 *       pair_offsets[n_polygons] their total.
 *   segger_polygon_join_fill   the same traversal again, with the same inputs and the workspace as the count call left
 *       it: writes the point ids of polygon p to point_index_out[pair_offsets[p] .. pair_offsets[p + 1]).  The slot of a
 *       pair is the polygon's offset + the number of matches before it in the traversal (ballot + prefix popcount), not
 *       an atomic: within a polygon the ids come in (cell row, cell, point id) order, the same from call to call.  Nothing
 *       is written at or beyond capacity entries, nor outside the polygon's own range.
 *   No floating-point atomics anywhere.
 *
 * Errors found on the device, without a synchronisation (the int32 at byte 0 of the workspace, 0 = none, valid once the
 *   stream has run; int32 words 1 and 2 are the polygons that took the register and the LDS route):
 *     SEGGER_PJOIN_ERR_OFFSETS  ring_offsets[p] < 0, ring_offsets[p + 1] < ring_offsets[p] or ring_offsets[p + 1] > n_vertices;
 *     SEGGER_PJOIN_ERR_CAP      a ring of more than SEGGER_MORPH_MAX_VERTS vertices (the Python wrapper refuses it before
 *                               the call, naming the polygon, as it does for segger_polygon_props);
 *     SEGGER_PJOIN_ERR_BUFFER   a negative, infinite or NaN buffer[p];
 *     SEGGER_PJOIN_ERR_FILL     the fill found other counts than pair_offsets holds, or more pairs than capacity.
 *   A polygon with one of the first three matches nothing; nothing is read or written out of bounds for any of them.
 *
 * Workspace: segger_polygon_join_workspace_bytes(n_points, n_polygons, nx, ny) = 256 + up(8 N) + up(16 N) +
 *   up(4 (nx ny + 1)) + 2 up(4 n_polygons) + the radix sort's storage, with N = max(n_points, 1) and up() rounding up to
 *   256; the sort's storage depends on N and nx ny only.  256-byte aligned.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative n_points, n_polygons, n_vertices,
 *   workspace_bytes or capacity, 2^31 - 1 points or polygons or more, nx or ny < 1 or nx ny >= 2^31 - 1, a cell side that is
 *   not positive and finite, an origin that is not finite, an unknown predicate, and for n_points > 0 and n_polygons > 0 a
 *   NULL pointer (buffer may be NULL = no buffer; xy may be NULL when n_vertices = 0), a misaligned pointer (points and xy:
 *   16 bytes), a workspace below segger_polygon_join_workspace_bytes (which itself returns the negative code for sizes out
 *   of range).  n_points = 0 or n_polygons = 0 returns SEGGER_OK without touching a pointer or the device: pair_offsets
 *   is NOT written, the caller knows it is all zeros.
 * ---------------------------------------------------------------------- */
#define SEGGER_PJOIN_CONTAINS 0
#define SEGGER_PJOIN_INTERSECTS 1
#define SEGGER_PJOIN_ERR_OFFSETS 1
#define SEGGER_PJOIN_ERR_CAP 2
#define SEGGER_PJOIN_ERR_BUFFER 4
#define SEGGER_PJOIN_ERR_FILL 8
int64_t segger_polygon_join_workspace_bytes(int64_t n_points, int64_t n_polygons, int32_t nx, int32_t ny);
int segger_polygon_join_count(const double* points /* [N, 2] */, int64_t n_points, const int64_t* ring_offsets,
                              const double* xy, int64_t n_polygons, int64_t n_vertices,
                              const double* buffer /* [P] fp64 or NULL = 0 */, int32_t predicate, double x0, double y0,
                              double cell, int32_t nx, int32_t ny, int64_t* pair_offsets /* [P + 1] */, void* workspace,
                              int64_t workspace_bytes, segger_stream_t stream);
int segger_polygon_join_fill(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy,
                             int64_t n_polygons, int64_t n_vertices, const double* buffer, int32_t predicate, double x0,
                             double y0, double cell, int32_t nx, int32_t ny, const int64_t* pair_offsets,
                             int64_t* point_index_out, int64_t capacity, void* workspace, int64_t workspace_bytes,
                             segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Cell boundary polygons: one ring per segmented cell, the convex hull of the cell's transcripts -- the reference's
 * generate_boundaries / cell_boundary with method="convex_hull" (src/segger/export/boundary.py:157-217), optionally rounded
 * by Chaikin corner cutting (boundary.py:42-54).  The reference's DEFAULT method, "delaunay" (boundary.py:57-154, the
 * outline of a pruned Delaunay triangulation), is segger_cell_outlines below, an entry point of its own; this one does not
 * route to it.  The kernels behind segger_amd.boundaries.cell_boundaries.
 * csrc/boundaries.hip.  Purely additive: two new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * Input:  xy [n_rows, 2] fp64 (16-byte aligned), cell [n_rows] int32, keep [n_rows] bytes or NULL (= all ones), and the
 *   cell id domain n_cells.  Row i is COUNTED iff 0 <= cell[i] < n_cells, keep[i] != 0 and both coordinates are finite.  A
 *   negative cell id means "unassigned" and is skipped silently, as is a row with keep[i] == 0 whatever else it holds.  A
 *   row with keep[i] != 0 and cell[i] >= n_cells adds one to counters[4], one with an id inside the domain and a NaN or
 *   infinite coordinate adds one to counters[5]; neither is used anywhere.  -0.0 is read as +0.0.
 *
 * Output, for the K cells that get a polygon, in ascending cell id:
 *     ring_offsets   [K + 1] int64   ring q is xy_out[ring_offsets[q] .. ring_offsets[q + 1]), open (no closing duplicate)
 *     xy_out         [V, 2] fp64     the rings; a CSR that segger_polygon_props and segger_polygon_join_* take as it is
 *     cell_ids       [K] int32       the cell of ring q
 *     n_transcripts  [K] int64       its counted rows (duplicates included)
 *     counters       [SEGGER_BOUNDARY_COUNTERS] uint64:  0 counted rows, 1 present cells (at least one counted row), 2 K,
 *                    3 V, 4 rows with a cell id >= n_cells, 5 rows with a non-finite coordinate, 6 cells the chunked route
 *                    refused, 7 the largest such cell id + 1
 *   The arrays are sized by the caller for the worst case: ring_offsets min(n_rows, n_cells) + 1, cell_ids and n_transcripts
 *   min(n_rows, n_cells), xy_out xy_capacity vertices; n_rows << smoothing vertices always suffice, and nothing is written
 *   at or beyond xy_capacity (the caller compares counters[3] with it).  A present cell whose hull has fewer than 3
 *   vertices -- fewer than 3 distinct points, or only collinear ones -- has no polygon: the reference's
 *   np.unique(points) < 3 -> None and its collinear case, where shapely's hull is no Polygon.  present - K cells dropped.
 *
 * Stages, on one stream without a host synchronisation (every size downstream of the keys is a device counter):
 *   keys     key = cell << 32 | row for a counted row, n_cells << 32 otherwise; one keys-only radix sort, stable by
 *            construction (the row is part of the key): a cell's rows are contiguous, in ascending row order;
 *   segments the first sorted position of every present cell (a stream compaction) and its length;
 *   hull     one wave per cell, the cells binned by route on the device: n <= 64 points in registers; 64 < n <=
 *            SEGGER_MORPH_MAX_VERTS staged in LDS; above that the chunked route: hull what is staged, move the hull to the
 *            front of LDS, stage the next SEGGER_MORPH_MAX_VERTS - h points, hull again, until the cell is consumed.  If a
 *            running hull has more than SEGGER_BOUNDARY_CHUNK_MAX_HULL vertices while points remain, the cell is refused
 *            (counters[6], [7]; no polygon): every round then stages at least half a buffer of new points.
 *            The march is segger_polygon_props': from the lowest (x, then y) point, counter-clockwise; the next vertex is
 *            the most clockwise point as seen from the current one, ties go to the larger distance, then to the lower
 *            index; a point equal to the current one never competes.  A point on a hull edge or equal to another point
 *            is never a hull vertex.  The products run on the coordinates as given minus the current vertex, fp64, FMA
 *            contraction off: exact when the coordinates are integers below 2^25 in magnitude (or share such a grid).
 *            The hull's vertices are copies of input coordinates, bit for bit;
 *   scan     K, V and the offsets: an exclusive scan of h << smoothing over the cells with h >= 3;
 *   emit     the rings.  With smoothing = s > 0, s Chaikin iterations as the reference writes them: out[2k] = 0.75 p[k] +
 *            0.25 p[k + 1], out[2k + 1] = 0.25 p[k] + 0.75 p[k + 1], indices cyclic, two products and one sum per
 *            coordinate, unfused, iterated: every output vertex is computed from the s + 1 hull vertices it depends on,
 *            level by level, with the operations numpy performs -- the same bits.  A ring of h vertices becomes h 2^s.
 *   No floating-point atomics.  The same rows in any order give the same bytes whenever the orientation products above are
 *   exact; with coordinates for which they round, points within rounding of a hull edge may be decided differently.
 *
 * Workspace: segger_cell_boundaries_workspace_bytes(n_rows, n_cells), 256-byte aligned: with N = max(n_rows, 1),
 *   C = max(min(n_rows, n_cells), 1) and up() rounding up to 256:  256 + 2 up(4 C) + up(4 (N / 4097 + 1)) + up(8 N) +
 *   up(16 N) + 4 up(4 C) + the storage of the sort and of the compaction.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative n_rows, workspace_bytes or xy_capacity,
 *   2^31 - 1 rows or more, n_cells outside 1 .. 2^31 - 1, smoothing outside 0 .. SEGGER_BOUNDARY_MAX_SMOOTHING, and for
 *   n_rows > 0 a NULL pointer (keep may be NULL; xy_out may be NULL when xy_capacity = 0), a misaligned pointer (xy and
 *   xy_out: 16 bytes), a workspace below the size above.  n_rows = 0 returns SEGGER_OK after checking counters and
 *   ring_offsets for NULL and launches nothing: the caller's zeroed counters and ring_offsets[0] = 0 stand.
 * ---------------------------------------------------------------------- */
#define SEGGER_BOUNDARY_MAX_SMOOTHING 6
#define SEGGER_BOUNDARY_CHUNK_MAX_HULL 2048   /* half of SEGGER_MORPH_MAX_VERTS */
#define SEGGER_BOUNDARY_COUNTERS 8
int64_t segger_cell_boundaries_workspace_bytes(int64_t n_rows, int64_t n_cells);
int segger_cell_boundaries(const double* xy /* [N, 2] */, const int32_t* cell, const uint8_t* keep /* or NULL */,
                           int64_t n_rows, int64_t n_cells, int32_t smoothing, int64_t* ring_offsets, double* xy_out,
                           int64_t xy_capacity, int32_t* cell_ids, int64_t* n_transcripts, uint64_t* counters,
                           void* workspace, int64_t workspace_bytes, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Concave cell outlines: one ring per segmented cell from the pruned Delaunay triangulation of the cell's transcripts --
 * the reference's generate_boundaries / cell_boundary with its DEFAULT method="delaunay" (_CellOutline,
 * src/segger/export/boundary.py:57-154), optionally rounded by Chaikin corner cutting.  The kernels behind
 * segger_amd.boundaries.cell_outlines, csrc/outlines.hip.  Purely additive: two new symbols, SEGGER_ABI_VERSION stays 32.
 * segger_cell_boundaries is unchanged; it does not route to this entry point.
 *
 * Input, output, the counted rows, the order of the cells, the sizes of the arrays and the workspace rule are those of
 * segger_cell_boundaries above, with `connectivity` (the reference's knob, default 2.0) in front of `smoothing`.  A ring is
 * open, counter-clockwise, starts at its lexicographically lowest vertex and lists EVERY vertex of the outline, collinear
 * ones included (shapely's polygonize does not simplify); a vertex is an input coordinate bit for bit (-0.0 as +0.0).
 *     counters [SEGGER_OUTLINE_COUNTERS] uint64: 0 .. 5 as above; 6 cells with more than SEGGER_OUTLINE_MAX_POINTS distinct
 *              points, 7 the largest such cell id + 1; 8 cells whose triangulation contradicted itself, 9 the largest such
 *              cell id + 1.  A cell counted in 6 or 8 gets no polygon.
 *
 * Stages per cell, one single-wave workgroup per cell with its whole state in LDS (68 bytes per point of capacity: 136 KB
 * for SEGGER_OUTLINE_MAX_POINTS = 2048, 17 KB on the route of the cells with at most 256 rows):
 *   points   sorted by (x, y), exact duplicates dropped, multiplicity > 1 remembered.  Fewer than 3 distinct points, or
 *            all collinear: no polygon (the reference's np.unique(points) < 3 -> None, and qhull's error -> None);
 *   Delaunay grown edge by edge from point 0 and its nearest neighbour: the apex of a directed edge a -> b is the point
 *            left of ab that no other such point's in-circle test beats.  orient2d and incircle run on coordinate
 *            differences in fp64, FMA contraction off: exact when the coordinates share a grid and span fewer than 2^11
 *            steps of it in the cell.  Co-circular points tie; the tie is broken towards the fan from the lowest vertex of
 *            the co-circular polygon, which need not be qhull's choice;
 *   d_max    the largest nearest-neighbour distance (_nn_max): per vertex the shortest incident Delaunay edge, 0 for a
 *            point with multiplicity > 1; lengths are sqrt(dx dx + dy dy);
 *   peel 1   remove a triangle with a rim edge longer than 2 connectivity d_max, to the fixed point;
 *   peel 2   remove a triangle with a rim edge e for which (length > 1.5 connectivity d_max and angle > 90) or
 *            angle > 180 - 11.25 / connectivity, angle = degrees(acos(clamp(u.v / (|u| |v| + 1e-12), -1, 1))) at the
 *            vertex opposite e.  Both predicates are static, so the fixed points do not depend on the order of removal;
 *   largest  the edge-connected components of the surviving triangles; the one of largest area is kept; equal areas: the
 *            one whose lowest vertex is lower, then the one found first (the reference's choice is GEOS's order and is
 *            not reproduced).  Nothing survives: no polygon;
 *   ring     the component's rim walked with the interior on the left; then `smoothing` Chaikin iterations as above.
 *            shapely's buffer(0) after the smoothing, which can alter a smoothed concave ring that touches itself, is
 *            not reproduced.
 * A cell with more than SEGGER_OUTLINE_MAX_POINTS distinct points is refused (counters[6], [7]) by this entry point; the
 * route through global memory for such cells is segger_cell_outlines_large below.  Every loop is bounded before it is entered: at most 2 n - 5 triangles,
 * 3 per triangle directed edges, rounds at most the triangle count, a ring walk of at most one step per directed edge;
 * a table that overflows or a walk past its bound -- possible only when rounded predicates contradict each other --
 * refuses the cell through counters[8], [9].
 *
 * Workspace: segger_cell_outlines_workspace_bytes(n_rows, n_cells), 256-byte aligned: with N, C and up() as above
 *   256 + 2 up(4 C) + up(8 N) + up(16 N) + 4 up(4 C) + the storage of the sort and of the compaction.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: everything segger_cell_boundaries rejects, and
 *   a connectivity that is not a finite number > 0.  n_rows = 0 returns SEGGER_OK as above.
 * ---------------------------------------------------------------------- */
#define SEGGER_OUTLINE_MAX_POINTS 2048   /* 68 B of LDS per point: 139264 of the 163840 B of a CU */
#define SEGGER_OUTLINE_COUNTERS 10
int64_t segger_cell_outlines_workspace_bytes(int64_t n_rows, int64_t n_cells);
int segger_cell_outlines(const double* xy /* [N, 2] */, const int32_t* cell, const uint8_t* keep /* or NULL */,
                         int64_t n_rows, int64_t n_cells, double connectivity, int32_t smoothing, int64_t* ring_offsets,
                         double* xy_out, int64_t xy_capacity, int32_t* cell_ids, int64_t* n_transcripts,
                         uint64_t* counters, void* workspace, int64_t workspace_bytes, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Concave cell outlines with a route through global memory for large cells: segger_cell_outlines plus two arguments, the
 * kernels behind segger_amd.boundaries.cell_outlines(large_cells="global"), csrc/outlines_large.hip.  Purely additive: two
 * new symbols, SEGGER_ABI_VERSION stays 32; segger_cell_outlines keeps its signature, its behaviour and its messages.
 *
 *     lds_max_points  0 .. SEGGER_OUTLINE_MAX_POINTS: a cell with more distinct points than this leaves the LDS routes for
 *                     the large route; 0 sends every cell there.  SEGGER_OUTLINE_MAX_POINTS is the value to pass; lower
 *                     ones exist to test and to time the large route on small cells.
 *     large_rows      0 .. n_rows: the caller's bound on the summed COUNTED ROWS (duplicates included) of the cells that
 *                     take the large route -- every cell with more than lds_max_points counted rows is a safe choice.  It
 *                     sizes the workspace.  A cell takes a slice of as many rows as it has with one atomic add when it is
 *                     routed; when the slices handed out would exceed large_rows, or the cell has more than 2^28 rows
 *                     (directed-edge ids and hash slots are 32-bit), the cell is refused through counters[6], [7] exactly
 *                     as segger_cell_outlines refuses it: no polygon, nothing read or written outside a slice, the other
 *                     cells unaffected.  Which cells are refused when large_rows is too small depends on the order in
 *                     which they arrive, and a refusal cascades: the row counter only grows (rows given back under a
 *                     slice handed out meanwhile would be handed out twice), so once one cell did not fit, every
 *                     large cell that arrives after it in the call is refused as well, even one that would have
 *                     fitted.  With a sufficient bound none is.
 *     counters [SEGGER_OUTLINE_LARGE_COUNTERS] uint64: 0 .. 9 as for segger_cell_outlines (6, 7 now count what is still
 *                     refused); 10 cells the large route handled, 11 their distinct points, 12 the rows of the slices
 *                     handed out.
 *
 * A ring has the same bytes whichever route produced it: the large route runs the six stages above with the same orient2d,
 * incircle and tie rule, the same seed, and adds a component's area in the same order.  It differs in how: one 256-thread
 * workgroup per cell with the cell's state in its slice and 32-bit vertex, edge and triangle ids; the rows sorted in the
 * slice by a bitonic network; the directed-edge hash open addressing over 8 slots per distinct point; and the apex search
 * pruned -- the points are sorted by x and a better apex lies inside or on the circle through the edge and the best apex
 * so far, so the search runs outward from the edge and stops at the circle's x-extent, computed with its rounding error
 * added, so that a point on the circle is still seen.  The work per triangle is a chain of dependent reads of global
 * memory: such a cell takes far longer than its share of an LDS cell's time (README has the figures), and the large
 * kernel starts when the LDS kernels are done.
 *
 * Workspace: segger_cell_outlines_large_workspace_bytes(n_rows, n_cells, large_rows): with R = max(large_rows, 1)
 *   segger_cell_outlines_workspace_bytes(n_rows, n_cells) + up(4 C) + up(8 C)                      the large list, its slices
 *   + up(16 R) + up(R) + 2 up(24 R) + up(6 R) + up(8 R) + up(64 R) + up(32 R)                      175 bytes per row:
 *   points, multiplicity flags, triangle vertices and twins (3 uint32 x 2 triangles each), predicate bits, labels, hash keys
 *   and hash ids.  Monotone in large_rows.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: everything segger_cell_outlines rejects,
 *   lds_max_points outside its range, large_rows negative or above n_rows.  n_rows = 0 returns SEGGER_OK as above.
 * NOT BUILT: overlapping the large cells with the small ones (one stream, the kernels run one after another); a sort of
 *   the rows that is not a bitonic network (O(n log^2 n) passes over the slice).
 * ---------------------------------------------------------------------- */
#define SEGGER_OUTLINE_LARGE_COUNTERS 13
int64_t segger_cell_outlines_large_workspace_bytes(int64_t n_rows, int64_t n_cells, int64_t large_rows);
int segger_cell_outlines_large(const double* xy /* [N, 2] */, const int32_t* cell, const uint8_t* keep /* or NULL */,
                               int64_t n_rows, int64_t n_cells, double connectivity, int32_t smoothing,
                               int64_t* ring_offsets, double* xy_out, int64_t xy_capacity, int32_t* cell_ids,
                               int64_t* n_transcripts, uint64_t* counters, void* workspace, int64_t workspace_bytes,
                               int32_t lds_max_points, int64_t large_rows, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Boundary polygons from a label image: per label the border with the most vertices, as a ring CSR -- the reference's
 * masks_to_contours (src/segger/io/utils.py:8-41: per label a regionprops crop, cv2.findContours(RETR_LIST,
 * CHAIN_APPROX_SIMPLE), the contour with the most vertices, dropped with <= 2) as its CosMx intake drives it
 * (src/segger/io/cosmx.py:79-107).  The kernels behind segger_amd.contours.label_contours, csrc/contours.hip.  Purely
 * additive: two new symbols, SEGGER_ABI_VERSION stays 32.
 *
 *     labels        [height, width] int32, row = y, column = x, 0 = background, every value in 0 .. max_label.
 *     compartment   NULL, or [height, width] uint8: a pixel counts as its label only if bit `code` of the 256-bit set
 *                   valid0 .. valid3 (bit c of word c / 64) is set -- np.where(np.isin(compartment, codes), labels, 0)
 *                   fused into the read; no masked image is written.
 *     max_label     0 .. SEGGER_CONTOUR_MAX_LABEL: sizes five int32 tables.  Ids may be sparse.
 *     scale, trans  a vertex (x, y) is written as (x * scale_x + trans_x, y * scale_y + trans_y), one multiplication and
 *                   one addition in fp64, not fused; the integer coordinates are exact before it.
 *     ring_offsets  [C + 1] int64, label_ids [C] int32, n_pixels [C] int64 with C = max(min(max_label, height * width), 1):
 *                   the kept labels ascending, the masked pixel count of each.  Entries past the kept count are untouched.
 *     xy_out        [xy_capacity, 2] fp64.  A vertex at or past xy_capacity is not written; counters[8] says so and
 *                   counters[2] is the capacity that suffices.  ring_offsets is complete either way.
 *     counters      [SEGGER_CONTOUR_COUNTERS] uint64: 0 labels present, 1 labels kept, 2 vertices, 3 labels dropped for
 *                   <= 2 points, 4 borders traced, 5 the longest ring, 6 labels whose winner shared its count with another
 *                   border (ties broken), 7 pixels with a label outside 0 .. max_label (they count as background), 8 the
 *                   overflow word: 1 when vertices > xy_capacity, 9 labels that took the global route.
 *
 * The result, exactly.  The foreground of label L is {labels == L} after the mask.  Its borders are those of Suzuki and
 * Abe's border following with 8-connected foreground: every outer and every hole border of every 8-connected component, each
 * a closed chain of border pixels.  The reference hands cv2 the transposed crop, so the raster scan is x-major (cv rows are
 * x, cv columns are y) and that order is used wherever an order matters.  CHAIN_APPROX_SIMPLE: a chain point is kept iff
 * the step into it differs from the step out of it, cyclically -- the tip of a one-pixel spur is kept, the pixels of the
 * spur appear twice in the chain, an isolated pixel is one point.  Per label the border with the most kept points wins,
 * hole borders included; among equal counts the one whose canonical start is smallest in the scan order (UNPINNED: the
 * reference takes the last in cv2's list order, which is not known here).  A label whose winner has <= 2 points is
 * dropped.  A ring starts at the border's first pixel in the x-major scan -- of the visits to that pixel the one whose
 * previous pixel comes first clockwise from "y - 1" -- and runs in the direction border following gives; it is open (no
 * closing duplicate) and may be longer than SEGGER_MORPH_MAX_VERTS: the CSR has no cap, the downstream units refuse such
 * a ring themselves.  UNPINNED: cv2 was never run; for an outer border this start is believed to be cv2's.
 * The same bytes from run to run, for any launch geometry and on either route: nothing floating-point happens before the
 * final conversion, and the atomics are integer min, max and add.
 *
 *     lds_max_bits  0 .. SEGGER_CONTOUR_LDS_BITS: a label whose crop, rows padded to 32 columns, has at most this many bits
 *                   is traced over a bit mask in LDS; a larger one over the image in global memory (slow: every probe is
 *                   a read of the image).  SEGGER_CONTOUR_LDS_BITS is the value to pass; 0 sends every label there.
 *
 * Workspace: segger_label_contours_workspace_bytes(height, width, max_label), 256-byte aligned: with up(x) = x rounded up
 *   to 256 and C as above:  5 up(4 (max_label + 1)) + 6 up(4 C) + the storage of the compaction.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative height or width, height * width >= 2^31,
 *   max_label outside 0 .. SEGGER_CONTOUR_MAX_LABEL, lds_max_bits outside its range, a scale or translation that is not
 *   finite, negative workspace_bytes or xy_capacity, NULL or misaligned pointers, a workspace that is too small.
 *   height * width = 0 or max_label = 0 returns SEGGER_OK and launches nothing: the caller's zeroed counters and
 *   ring_offsets[0] stand.
 * The reference's simplify(tolerance) and is_valid that follow are segger_simplify_rings_* and segger_rings_simple below.
 * The first repair of fix_invalid_geometry, resort_coordinates, is segger_rings_resort.
 * NOT BUILT: TIFF reading, the buffer(0) repair of fix_invalid_geometry, the id strings, FOV stitching.
 * ---------------------------------------------------------------------- */
#define SEGGER_CONTOUR_MAX_LABEL (1 << 24)  /* five int32 tables of max_label + 1 entries: 320 MB at the cap */
#define SEGGER_CONTOUR_LDS_BITS 32768       /* 4 KB of LDS per single-wave workgroup: 32 of them fit a CU */
#define SEGGER_CONTOUR_COUNTERS 10
int64_t segger_label_contours_workspace_bytes(int64_t height, int64_t width, int64_t max_label);
int segger_label_contours(const int32_t* labels /* [H, W] */, const uint8_t* compartment /* [H, W] or NULL */,
                          uint64_t valid0, uint64_t valid1, uint64_t valid2, uint64_t valid3, int64_t height,
                          int64_t width, int64_t max_label, double scale_x, double scale_y, double trans_x,
                          double trans_y, int64_t* ring_offsets, double* xy_out, int64_t xy_capacity, int32_t* label_ids,
                          int64_t* n_pixels, uint64_t* counters, void* workspace, int64_t workspace_bytes,
                          int32_t lds_max_bits, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Ring simplification and validity on a ring CSR: what the reference's CosMx intake does right after masks_to_contours,
 * `geometry.simplify(tolerance)` (src/segger/io/cosmx.py:94-96, GEOS's topology-preserving simplifier, per polygon), and
 * the `is_valid` that fix_invalid_geometry asks first (io/utils.py:127-136; io/preprocessor.py:472).  The kernels behind
 * segger_amd.simplify.simplify_rings / rings_simple, csrc/simplify.hip.  Purely additive: four new symbols,
 * SEGGER_ABI_VERSION stays 32.
 *
 * The arithmetic.  A ring is xy[off[p] .. off[p + 1]) as segger_polygon_props takes it: either orientation, a closing
 * duplicate of its first vertex dropped bit for bit, n open vertices v_0 .. v_(n-1), index n meaning v_0.  Everything is
 * fp64 on the ring translated to its first vertex (v_k = xy_k - xy_0, one subtraction) before any product, no FMA
 * contraction.  Coordinates are finite.
 *   dist2(v; a, b), the squared distance from v to the closed segment (a, b), is segger_polygon_join_*'s, in its order:
 *     e = b - a, w = v - a, cr = e.x w.y - e.y w.x, dot = w.x e.x + w.y e.y, len2 = e.x e.x + e.y e.y;
 *     dist2 = w.x w.x + w.y w.y if dot <= 0 or len2 == 0;  |v - b|^2 (the same form) if dot >= len2;  cr cr / len2 otherwise.
 *   orient(a, b, c) is the sign of (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x) as computed.
 *   touch(s, t) of two closed segments s = (a, b), t = (c, d): true when they share a point, unless what they share is a
 *     single point that is an endpoint of both.  A collinear overlap longer than a point is a touch, an endpoint in the
 *     other segment's interior is a touch, a zero-length segment is a point.  As computed, without a division:
 *       o1 = orient(a, b, c), o2 = orient(a, b, d), o3 = orient(c, d, a), o4 = orient(c, d, b);
 *       in(o, p; q, r) = o == 0, p within the coordinate intervals of q and r, p != q and p != r;
 *       touch = (o1 o2 < 0 and o3 o4 < 0) or in(o1, c; a, b) or in(o2, d; a, b) or in(o3, a; c, d) or in(o4, b; c, d)
 *               or (a != b and {a, b} == {c, d}).
 *     With coordinates whose translated differences are integers below 2^26 every orient is exact and touch is the
 *     geometric statement.
 *
 * segger_simplify_rings_*: Douglas-Peucker over the closed sequence v_0 .. v_(n-1), v_0 of a ring of n >= 3 -- n input
 * edges e_k = (v_k, v_(k+1)), root section (0, n) -- depth first, left before right.  A section (i, j) with j == i + 1
 * emits its input edge.  Otherwise m is the interior index with the largest dist2(v_k; v_i, v_j), the lowest index among
 * equals, and the section is FLATTENED (the chord (v_i, v_j) is emitted, the interior dropped) iff
 *   (a) dist2(v_m; v_i, v_j) <= tol * tol, and
 *   (b) with preserve_topology: the chord touches no input edge outside the section (e_k, k < i or k >= j) and no chord
 *       emitted so far -- which, the walk being left first, are exactly the consecutive pairs of the kept vertices with
 *       index <= i;
 * otherwise it is split at m.  Vertex 0 is always kept; the kept vertices are the section ends.  The chord back over an
 * emitted chord is a touch and is refused, so after a split of the root at least three vertices stay and no minimum-size
 * rule is needed; without preserve_topology (b) is dropped and this is the classical algorithm.  In either mode a ring that
 * comes out with fewer than 3 vertices -- with the guard only when the root itself is flattened, every vertex within tol of
 * v_0 and nothing yet to touch -- is returned as it went in and counted.  A ring of fewer than 3 open vertices passes
 * through.  Output rings are open: the n open vertices of a ring passed through or restored, the kept ones otherwise, as
 * the INPUT's bytes (untranslated), with the index into xy of each.
 *
 * UNPINNED.  GEOS could not be run where this was written and the reference was never run.  GEOS's
 * TopologyPreservingSimplifier has this structure (farthest point; a candidate segment refused when it has an interior
 * intersection with input or output segments; depth-first recursion); three of its details are NOT reproduced and may
 * differ between GEOS versions: its minimum-size rule at shallow depth, its optional removal of the ring's endpoint, and
 * its "jump" check.  Its output may therefore differ from this one in single vertices.  Downstream code accepts any start.
 *
 *   _mark     tolerance: fp64 on the device, finite and >= 0; tolerance_stride 0 = one value for all, 1 = one per polygon.
 *             small_max_verts 0 .. SEGGER_SIMPLIFY_SMALL_VERTS: a ring of at most this many vertices runs in the small
 *             LDS tier (4864 B per single-wave workgroup), a longer one in the large (77824 B, two per CU); the same code,
 *             the same bytes; SEGGER_SIMPLIFY_SMALL_VERTS is the value to pass, 0 sends every ring to the large tier.
 *             Writes out_offsets [n_polygons + 1] (the output CSR) and counters [SEGGER_SIMPLIFY_COUNTERS] int64:
 *             0 vertices in (open), 1 vertices out, 2 sections visited (single edges included), 3 chords refused by the
 *             guard, 4 rings passed through, 5 rings restored after collapse, 6 the longest output ring, 7 the error word:
 *             SEGGER_MORPH_ERR_OFFSETS / _CAP as segger_polygon_props sets them, SEGGER_SIMPLIFY_ERR_TOL for a tolerance
 *             that is negative or not finite; such a ring gets no output vertices.  The keep mask stays in the workspace.
 *   _emit     after _mark, same workspace: xy_out [capacity, 2] fp64 and vertex_index [capacity] int64, capacity >=
 *             counters[1]; nothing is written at or past capacity.
 * segger_rings_simple: ok [n_polygons] uint8 and reason [n_polygons, 3] int32 = (code, i, j).  A ring is simple iff at
 * least 3 vertices are left when consecutive duplicates are dropped (cyclically; otherwise SEGGER_RING_TOO_FEW, -1, -1)
 * and no two of its edges e_i, e_j, i < j, touch (otherwise SEGGER_RING_TOUCH and the lowest such pair in (i, j) order,
 * indices into the open ring as given, duplicates not dropped).  Adjacent edges share their common endpoint, which touch
 * allows; a fold-back is a touch.  This is what is_valid asks of a single-shell polygon.  The error word is the first
 * int32 of the workspace.
 *
 * Workspace, 256-byte aligned, with up(x) = x rounded up to 256: segger_simplify_rings_workspace_bytes(P, V) =
 *   256 + 2 up(4 P) + up(16 P) + up(V); segger_rings_simple needs (P, 0).
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative sizes, 2^31 - 1 polygons or more, a
 *   stride or small_max_verts outside its range, NULL or misaligned pointers, a workspace that is too small.
 *   n_polygons = 0 returns SEGGER_OK and launches nothing.  No scratch, no atomics on floats: the same bytes from run to
 *   run and for any order of the polygons in the CSR.
 * The repair that fix_invalid_geometry tries on the rings that are not simple, resort_coordinates, is segger_rings_resort
 * below.  NOT BUILT: the buffer(0) repair, holes and multi-part polygons, rings above SEGGER_MORPH_MAX_VERTS.
 * ---------------------------------------------------------------------- */
#define SEGGER_SIMPLIFY_SMALL_VERTS 256
#define SEGGER_SIMPLIFY_COUNTERS 8
#define SEGGER_SIMPLIFY_ERR_TOL 4
#define SEGGER_RING_OK 0
#define SEGGER_RING_TOO_FEW 1
#define SEGGER_RING_TOUCH 2
int64_t segger_simplify_rings_workspace_bytes(int64_t n_polygons, int64_t n_vertices);
int segger_simplify_rings_mark(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                               const double* tolerance, int64_t tolerance_stride, int32_t preserve_topology,
                               int32_t small_max_verts, int64_t* out_offsets, int64_t* counters, void* workspace,
                               int64_t workspace_bytes, segger_stream_t stream);
int segger_simplify_rings_emit(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                               const int64_t* out_offsets, double* xy_out, int64_t* vertex_index, int64_t capacity,
                               void* workspace, int64_t workspace_bytes, segger_stream_t stream);
int segger_rings_simple(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices, uint8_t* ok,
                        int32_t* reason, int32_t small_max_verts, void* workspace, int64_t workspace_bytes,
                        segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Ring repair on a ring CSR: the first repair of the reference's fix_invalid_geometry (src/segger/io/utils.py:127-159,
 * called for every boundary intake at io/preprocessor.py:311, :316 and :472), resort_coordinates (io/utils.py:83-102) --
 * the vertices of the closed coordinate sequence re-sorted by np.arctan2 around their mean -- for the rings a mask
 * selects.  The kernel behind segger_amd.repair.resort_rings / repair_rings, csrc/repair.hip.  Purely additive: one new
 * symbol, SEGGER_ABI_VERSION stays 32.
 *
 * A ring is xy[off[p] .. off[p + 1]) as segger_rings_simple takes it, n open vertices v_0 .. v_(n-1).  A ring keeps its
 * vertex count, so ring_offsets is the output's too.  A ring that is not selected, or has fewer than 3 open vertices, and
 * every row of xy outside the rings is copied through bit for bit with vertex_index the row itself.  For a selected ring:
 *   centre   c = (sum_{k<n} v_k + v_0) / (n + 1) per coordinate in fp64 -- the reference sorts the CLOSED sequence, so
 *            vertex 0 counts twice.  The order of the sum: 64 partial sums s_l = ((0 + v_l) + v_(l+64)) + v_(l+128) + ...
 *            (ascending k, starting from +0; s_l = 0 where l >= n), then six rounds m = 1, 2, 4, 8, 16, 32 of
 *            s_l <- s_l + s_(l xor m) for every l at once; then (s_0 + v_0) / (n + 1), one addition and one division.
 *            The centre is never returned: only the order depends on it.
 *   d_k      = (fl(x_k - c_x), fl(y_k - c_y)), the rounded differences the reference hands to arctan2.
 *   order    ascending EXACT angle of d_k in (-pi, pi] with arctan2's conventions: d = (0, 0) has angle 0; d_y = 0 (either
 *            zero), d_x < 0 has angle +pi and comes last.  Vertices at one exact angle go by ascending squared length of
 *            d, compared exactly (at one angle that is the order of |d_x|, or of |d_y| where d_x = 0), then by ascending
 *            input index.  The result is counter-clockwise around c and starts at the first vertex past the negative-x ray.
 *            The reference's closing duplicate is not emitted: it would sit next to its twin and add nothing.
 *   exact    the comparator is the half-plane class of d (d_y < 0; angle 0; d_y > 0; angle pi) and, within a class, the
 *            sign of d_a x d_b = a_x b_y - a_y b_x obtained without rounding: each product as its rounded value plus the
 *            FMA's error term, the four terms summed into a non-overlapping expansion whose highest non-zero component
 *            carries the sign.  Neither a float64 atan2 key nor a float64 cross product: both mis-order vertices whose
 *            angles differ by less than their rounding (tests/repair_cases.py holds such pairs).  Exact while every
 *            non-zero |d_x|, |d_y| lies in 2^-480 .. 2^480 (no product overflows, every error term is representable);
 *            coordinates are finite.  With coordinates that are not numbers the output is still a permutation of the ring.
 *   closed   a ring GIVEN with a closing duplicate (n + 1 entries) keeps its n + 1 entries: c and the d_k are as above, the
 *            duplicate has d_0 and index n and is therefore emitted after vertex 0 and after every vertex with the same d.
 * Writes xy_out [n_vertices, 2] fp64 (the INPUT's bytes; xy_out must not be xy) and vertex_index [n_vertices] int64, the
 * row of xy each output row came from: xy_out = xy[vertex_index], a permutation within every ring.
 *   select   uint8 [n_polygons], non-zero = re-sort this ring; NULL = all.  Every ring's offsets are checked, selected or not.
 *   small_max_verts  as segger_rings_simple: a ring of at most this many vertices runs in the small LDS tier (4608 B per
 *            single-wave workgroup: the differences 16 B and an index 2 B a vertex), a longer one in the large (73728 B,
 *            two per CU); the same code, the same bytes; SEGGER_SIMPLIFY_SMALL_VERTS is the value to pass.
 * One single-wave workgroup per selected ring sorts the vertex indices in LDS with a bitonic network over the padded size.
 * The error word is the first int32 of the workspace: SEGGER_MORPH_ERR_OFFSETS / _CAP as segger_polygon_props sets them
 * (a ring above SEGGER_MORPH_MAX_VERTS is refused); such a ring is copied through.
 *
 * Workspace, 256-byte aligned: 256 + 2 up(4 P) bytes; segger_simplify_rings_workspace_bytes(P, 0) is enough and is what
 *   the Python side passes.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative sizes, 2^31 - 1 polygons or more, a
 *   small_max_verts outside its range, NULL or misaligned pointers, xy_out == xy, a workspace that is too small.
 *   n_polygons = 0 returns SEGGER_OK and launches nothing (xy_out and vertex_index are not written).  No scratch, no
 *   atomics on floats: the same bytes from run to run, for any order of the polygons in the CSR and on either tier.
 * UNPINNED against numpy where float64 arctan2 values tie or invert by rounding: np.argsort is not stable there and the
 *   reference's order among such vertices is whatever its sort does; the exact order above is this project's contract.
 * NOT BUILT: the buffer(0) fallback that fix_invalid_geometry takes when the re-sorted ring is still invalid, with its
 *   largest-component rule (GEOS's answer on a self-crossing ring depends on winding, and GEOS could not be run); holes
 *   and multi-part polygons; rings above SEGGER_MORPH_MAX_VERTS.
 * ---------------------------------------------------------------------- */
int segger_rings_resort(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                        const uint8_t* select /* [n_polygons] or NULL = all */, double* xy_out, int64_t* vertex_index,
                        int32_t small_max_verts, void* workspace, int64_t workspace_bytes, segger_stream_t stream);

/* ------------------------------------------------------------------------
 * Polygon overlap join of two ring CSRs A and B: every pair (a, b) whose closed polygons share a point, and the area of
 * their intersection -- the reference's polygons_in_polygons (src/segger/geometry/query.py:244-285, a CPU gpd.sjoin with
 * predicate='intersects', called from data/tiling.py:134) and what a comparison of a segmentation with a vendor's needs
 * (IoU per cell).  The kernels behind segger_amd.overlap.polygon_overlaps / polygons_in_polygons, csrc/polygon_overlap.hip.
 * Purely additive: three new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * Polygons are single exterior rings, xy[off[p] .. off[p + 1]) as segger_polygon_props takes them: either orientation, a
 * closing duplicate of the first vertex dropped bit for bit, a ring above SEGGER_MORPH_MAX_VERTS refused through the
 * set's error word (A's is int32 word 0 of the workspace, B's is word 8; SEGGER_MORPH_ERR_OFFSETS / _CAP).  A ring with
 * fewer than 3 open vertices pairs with nothing.  Coordinates are finite.
 *
 * The area, measure-theoretically, so that shared edges, collinear overlaps, nesting and self-overlap are no special
 * cases.  For ring A with s_A the sign of its shoelace sum and an edge e = (p -> q) with p.x != q.x let
 * sigma_e = s_A sign(p.x - q.x).  With a baseline y0 not above any vertex of the pair,
 *     1_A(x, y) = sum over e of sigma_e [x in the half-open x-range of e] [y0 <= y < y_e(x)]      almost everywhere
 * (vertical edges contribute nothing), hence
 *     area(A and B) = sum over e in A, f in B of sigma_e sigma_f I(e, f),
 *     I(e, f) = the integral of min(y_e(x), y_f(x)) - y0 over the overlap [xl, xr] of the two x-ranges:
 * one trapezoid, or two split at the single crossing of the two lines.  (For a ring that winds twice round a region 1_A is
 * 2 there: the sum is then the integral of 1_A 1_B, which is what "area" means for such a ring here.)
 * As computed: fp64, no FMA contraction, BOTH rings translated to the first vertex of ring A before any product, y0 the
 * lowest translated y of the pair;  y_e(x) = p.y (q.y) when x == p.x (q.x), else p.y + (x - p.x) * ((q.y - p.y) / (q.x - p.x));
 * el, er, fl, fr the two lines at xl and xr, w = xr - xl, ml = min(el, fl) - y0, mr = min(er, fr) - y0;  when el - fl and
 * er - fr have strictly opposite signs t = (el - fl) / ((el - fl) - (er - fr)), mc = (el + t (er - el)) - y0 and
 * I = 0.5 w (t (ml + mc) + (1 - t) (mc + mr)), otherwise I = 0.5 w (ml + mr).  Edge pair (k of A, l of B) has index
 * t = k n_b + l and belongs to lane t mod 64; a lane adds its terms in increasing t from +0.0 (a pair whose closed x-ranges
 * are apart is skipped: its term is zero); the 64 sums are combined by the xor butterfly at distances 1, 2, .. 32.  The
 * result is 0 when the predicate below is false, and otherwise clamped into [0, min(area_a[a], area_b[b])].  The bits are
 * the same from run to run, for any order of the polygons in either set, for any grid and on every tier.
 *   Error: a term carries at most 16 u W H absolute error (u = 2^-53; W, H the pair's joint extent) and the summation of T
 *   non-zero terms at most (T - 1) u S, S the sum of their magnitudes: |area - exact| <= 2^-52 (T S + 16 T W H).
 *
 * The predicate: intersects(A, B) iff some edge of A and some edge of B share a point (closed segments: with o1 .. o4 the
 * four orient() of segger_rings_simple's touch, (o1 o2 < 0 and o3 o4 < 0) or an o_i == 0 whose point lies within the
 * coordinate intervals of the other segment -- touch WITHOUT its shared-endpoint exemption), or vertex 0 of A is inside B
 * by segger_polygon_join_*'s half-open parity rule, or vertex 0 of B is inside A.  Exact for coordinates whose translated
 * differences are integers below 2^26.  This is GEOS's 'intersects' for valid rings; what GEOS answers for invalid rings
 * is UNPINNED (it was never run).
 *
 * Candidates: every (a, b), both of 3 or more vertices, whose closed bounding boxes overlap -- found over a uniform grid
 * of nx x ny cells of side `cell` from (x0, y0) (coordinates outside are clamped into the border cells), B binned, A
 * walking: a pair is emitted only in the cell (max(cx0_a, cx0_b), max(cy0_a, cy0_b)), the cell of the lower-left corner
 * of the two boxes' intersection, so once.  A polygon whose box covers more than SEGGER_OVERLAP_WIDE_CELLS cells is "wide"
 * and is tested against every polygon of the other set instead.  The grid decides the speed and nothing else: the SET of
 * candidates is the same for any grid; their order in `candidates` is unspecified.
 *
 *   _candidates  bins both sets, builds the grid, counts: writes *n_candidates (int64, device) and keeps its tables in the
 *                workspace for _pairs.  Zeroes the workspace's words.
 *   _pairs       after _candidates, same arguments and workspace, capacity >= *n_candidates: writes candidates [capacity]
 *                int64 = a << 32 | b, intersects [capacity] uint8 and area [capacity] fp64 (nothing at or past capacity, nothing
 *                past *n_candidates).  area_a [Pa], area_b [Pb]: the polygons' areas for the clamp (segger_polygon_props'), or
 *                both NULL for no upper clamp.  Tiers by n = max(n_a, n_b): n <= reg_max_verts (0 .. 64) both rings in
 *                registers, no LDS; n <= small_max_verts (0 .. SEGGER_OVERLAP_SMALL_VERTS) both in the LDS of a
 *                single-wave workgroup, 8192 B; otherwise 131072 B, one workgroup per CU.  64 and
 *                SEGGER_OVERLAP_SMALL_VERTS are the values to pass; 0, 0 sends every pair to the large tier (tests and
 *                timing).  int32 word 16 of the workspace counts the pairs that took an LDS tier.
 * Workspace, 256-byte aligned, with up(x) = x rounded up to 256 and C = nx ny: segger_polygon_overlap_workspace_bytes(Pa, Pb,
 *   nx, ny) = 256 + 2 up(4 Pa) + 2 up(4 Pb) + up(32 Pa) + up(32 Pb) + up(16 Pa) + up(16 Pb) + up(4 Pa) + up(4 Pb) +
 *   up(4 (C + 1)) + up(4 C) + up(4 SEGGER_OVERLAP_WIDE_CELLS Pb) + up(8 (Pa + Pb + 1)).  Monotone in every argument.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative sizes, 2^31 / SEGGER_OVERLAP_WIDE_CELLS
 *   polygons or more in a set, a bad grid, a tier bound outside its range, NULL or misaligned pointers, a workspace that is
 *   too small.  An empty set on either side returns SEGGER_OK and launches nothing.  No scratch, no atomics on floats.
 * NOT BUILT: predicate 'contains' (deciding it exactly needs the sub-segments of an edge between boundary touches), the
 *   intersection polygon itself, holes, multi-part polygons.
 * ---------------------------------------------------------------------- */
#define SEGGER_OVERLAP_SMALL_VERTS 256
#define SEGGER_OVERLAP_WIDE_CELLS 64
int64_t segger_polygon_overlap_workspace_bytes(int64_t n_polygons_a, int64_t n_polygons_b, int32_t nx, int32_t ny);
int segger_polygon_overlap_candidates(const int64_t* ring_offsets_a, const double* xy_a, int64_t n_polygons_a,
                                      int64_t n_vertices_a, const int64_t* ring_offsets_b, const double* xy_b,
                                      int64_t n_polygons_b, int64_t n_vertices_b, double x0, double y0, double cell, int32_t nx,
                                      int32_t ny, int64_t* n_candidates, void* workspace, int64_t workspace_bytes,
                                      segger_stream_t stream);
int segger_polygon_overlap_pairs(const int64_t* ring_offsets_a, const double* xy_a, int64_t n_polygons_a, int64_t n_vertices_a,
                                 const int64_t* ring_offsets_b, const double* xy_b, int64_t n_polygons_b, int64_t n_vertices_b,
                                 double x0, double y0, double cell, int32_t nx, int32_t ny, const double* area_a,
                                 const double* area_b, const int64_t* n_candidates, int64_t* candidates, uint8_t* intersects,
                                 double* area, int64_t capacity, int32_t reg_max_verts, int32_t small_max_verts, void* workspace,
                                 int64_t workspace_bytes, segger_stream_t stream);

/* ----------------------------------------------------------------------
 * Fragment cells (csrc/fragments.hip; segger_amd.fragments): connected components of the unassigned
 * transcripts over the transcript-graph edges whose embeddings agree.  Upstream segger calls this "fragment mode"
 * (use_cc); the reference snapshot this project follows does not contain it, so the contract below is this project's own
 * and is UNPINNED by any reference run.
 *
 * State: parent [n_transcripts] int32, initialised by the caller to the identity (parent[i] = i), and counters
 * [SEGGER_FRAGMENTS_COUNTERS] int64, zeroed by the caller: 0 edges seen, 1 live edges, 2 kept edges, 3 edges with an id
 * out of range (all four summed over the updates), 4 candidates (unassigned transcripts), 5 components (singletons
 * included), 6 fragments, 7 candidates whose parent chain held a value these kernels cannot have written (4 .. 7 are set by
 * _finalize).
 *
 *   _update    one launch, enqueue only.  Edge e = (src[e], dst[e]), local ids of one batch of n_nodes rows; tx_index
 *              [n_nodes] int64 maps a local id to its transcript (NULL: the identity); mask [n_nodes] uint8 (NULL: all
 *              true); unassigned [n_transcripts] uint8.  An edge with a local id outside [0, n_nodes), or -- its source's
 *              mask being true -- a transcript id outside [0, n_transcripts), is counted (counter 3) and takes part in
 *              nothing: no such id is ever an address.  An edge is LIVE when mask[src] is true, both transcripts are
 *              unassigned and differ, and edge_keep[e] (uint8, NULL: all true) is non-zero.  A live edge is KEPT when
 *                z != NULL:           sim >= min_similarity with sim = dot / (max(sqrt(aa), 1e-8f) * max(sqrt(bb), 1e-8f)),
 *                                     dot, aa, bb the three sums over the `channels` stored values of rows src and dst of z
 *                                     ([n_nodes, channels] in `dtype`, row stride ld_z elements) accumulated in fp32 (fused
 *                                     multiply-adds, lane partial sums combined by a tree); sqrt, the multiply and the divide
 *                                     are correctly rounded fp32 -- so |sim - exact cosine of the stored values| <=
 *                                     (2 channels + 6) 2^-24, and a cosine of small-integer rows is exact;
 *                similarity != NULL:  similarity[e] >= min_similarity (fp32, exact; no row is read);
 *                neither:             always.
 *              NaN is never >= anything: not kept.  The endpoints of a kept edge are united in `parent`: the larger root is
 *              hooked under the smaller by an agent-scope compare-and-swap, so parent[i] <= i throughout and the root of a
 *              component is its smallest transcript.  Rows that are whole 16-byte pieces (base, ld_z and channels) are read
 *              16 bytes a lane; any other shape an element a lane.
 *   _finalize  flattens parent (parent[i] = root of i for every candidate; further updates may follow), counts the members
 *              of every root, and writes fragment [n_transcripts] int64 = first_id + rank for the members of a component of
 *              min_size members or more, -1 for everything else, where rank numbers those components by their smallest
 *              transcript, ascending; root [capacity] and size [capacity] int32 per fragment in rank order (nothing at or
 *              past capacity; n_transcripts / min_size always suffices).  Workspace, 256-byte aligned, with up(x) = x
 *              rounded up to 256: up(4 n_transcripts) + up(8 (ceil(n_transcripts / SEGGER_FRAGMENTS_CHUNK) + 1)) bytes.
 * Every output is a function of the SET of kept edges: not of the order of edges, batches or atomics.  No scratch, integer
 * atomics only.  Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative sizes, n_transcripts
 * outside [1, 2^31), 2^31 nodes or more, channels outside 1 .. SEGGER_FRAGMENTS_MAX_CHANNELS, an unknown dtype, both z and
 * similarity, a NaN min_similarity, min_size < 1, a negative first_id or capacity, NULL or misaligned pointers, a workspace
 * that is too small.  n_edges = 0 returns SEGGER_OK and launches nothing.
 * ---------------------------------------------------------------------- */
#define SEGGER_FRAGMENTS_COUNTERS 8
#define SEGGER_FRAGMENTS_CHUNK 2048
#define SEGGER_FRAGMENTS_MAX_CHANNELS 1024
int segger_fragments_update(const void* z, int64_t ld_z, int32_t channels, int32_t dtype, const float* similarity,
                            const uint8_t* edge_keep, const int64_t* src, const int64_t* dst, int64_t n_edges,
                            const int64_t* tx_index, const uint8_t* mask, int64_t n_nodes, const uint8_t* unassigned,
                            int64_t n_transcripts, float min_similarity, int32_t* parent, int64_t* counters,
                            segger_stream_t stream);
int segger_fragments_finalize(int32_t* parent, const uint8_t* unassigned, int64_t n_transcripts, int64_t min_size,
                              int64_t first_id, int64_t* fragment, int32_t* root, int32_t* size, int64_t capacity,
                              int64_t* counters, void* workspace, int64_t workspace_bytes, segger_stream_t stream);

/* ----------------------------------------------------------------------
 * Buffered-boundary count matrices (csrc/buffered_counts.hip; segger_amd.buffered_counts): the polygon x gene
 * count matrix of boundaries grown by a distance -- the reference's get_buffered_counts -> buffer_polygons ->
 * get_expression_matrix (src/segger/metrics/segment.py), the nucleus-expansion baseline -- as a CSR, without the pair list.
 * The join of segger_polygon_join_* and the histogram of segger_expression_build fused: one wave owns one polygon and builds
 * the polygon's gene histogram in LDS where the hits are found.  A point inside several grown polygons is counted in each.
 * Purely additive: three new symbols, SEGGER_ABI_VERSION stays 32.
 *
 * The predicate, the arithmetic, the rings (a CSR of single exterior rings in fp64, a closing duplicate dropped, fewer than
 *   3 vertices match nothing, at most SEGGER_MORPH_MAX_VERTS), the uniform grid, the walk and its margin are
 *   segger_polygon_join_*'s above, bit for bit: both units compile csrc/ring_predicate.h and csrc/join_grid.h.
 *
 * Inputs beyond the join's:  gene [n_points] int32, the gene of every point;  n_genes, 1 .. SEGGER_BCOUNT_MAX_GENES.  A point
 *   whose gene lies outside [0, n_genes) is never an index: when it matches a polygon it is counted in n_bad (once per
 *   polygon it matches) and in n_pairs, and takes part in nothing else.
 *
 * Two calls (the size of the result is known on the device only):
 *   segger_buffered_counts_count  bins the points (keys, cell starts, cell-ordered points, and gene in cell order beside
 *       them) and the polygons (by route), then per polygon p writes the number of distinct in-range genes it hits to
 *       indptr[p + 1] and the number of matched in-range points to cell_count[p], and scans indptr on the device:
 *         indptr     [n_polygons + 1] int64   row offsets, indptr[n_polygons] = nnz <= min(n_pairs, n_polygons n_genes);
 *         cell_count [n_polygons]     int64   = the sum of the row's counts, <= n_points;
 *         counters   [SEGGER_BCOUNT_COUNTERS] int64 (zeroed by the call):  0 n_pairs, the matched (point, polygon) pairs,
 *                    out-of-range genes included;  1 nnz;  2 n_bad;  3 n_overflow_rows, the polygons with more than
 *                    SEGGER_BCOUNT_TOUCHED distinct genes;  4 n_large_tier, the polygons (of 3 or more vertices) that ran
 *                    on the large tier: all of them when n_genes > SEGGER_BCOUNT_SMALL_GENES, none otherwise.
 *   segger_buffered_counts_fill   the same traversal again, with the same inputs and the workspace as the count call left
 *       it, indptr and cell_count as it wrote them: writes indices (the gene id, strictly ascending inside a row) and
 *       counts (int32, >= 1) at indptr[p] .. indptr[p + 1).  Nothing is written at or beyond capacity entries, nor outside the polygon's own row.
 *
 * The histogram.  int32 hist[n_genes] per wave in LDS, zero between polygons.  A hit is an LDS atomic add on its gene; the
 *   lane that sees the old value 0 appends the gene to the wave's touched list (SEGGER_BCOUNT_TOUCHED entries, the slot from
 *   a ballot).  After the walk the touched list is sorted (csrc/wave_sort.h, the bitonic network of segger_rings_resort),
 *   the row is written from it and exactly those entries of hist are zeroed: the cost of a polygon does not grow with
 *   n_genes.  A polygon with more distinct genes than the list holds is written by one ordered scan of hist instead
 *   (n_overflow_rows).  Two tiers:
 *     small  n_genes <= SEGGER_BCOUNT_SMALL_GENES: 8 KB of hist and 2 KB of list a wave; rings of n <= 64 vertices in
 *            registers, four waves a workgroup (40 KB); longer rings one single-wave workgroup with the 64 KB ring stage
 *            (74 KB, two a CU);
 *     large  n_genes <= SEGGER_BCOUNT_MAX_GENES: one single-wave workgroup per polygon, the whole histogram in LDS.
 *   SEGGER_BCOUNT_MAX_GENES = (SEGGER_BCOUNT_LDS_BYTES - 65536 - 4 SEGGER_BCOUNT_TOUCHED) / 4 = (163840 - 65536 - 2048) / 4
 *   = 24064: the 160 KB of LDS a CDNA4 workgroup can address, minus the 64 KB ring stage of the long-ring route, minus the
 *   touched list, in int32 entries.  Larger panels need a key-sort route, which is NOT BUILT; nor is a histogram sized by
 *   n_genes (every panel above SEGGER_BCOUNT_SMALL_GENES runs one wave a workgroup).
 *   Integer atomics only, no floating-point accumulation, no scratch.  Every output is a function of the inputs alone -- the
 *   sums are integers and the rows are sorted -- the same bytes for any grid, any launch geometry and either tier.
 *
 * Errors found on the device (the int32 at byte 0 of the workspace, as the join's; the bits are the join's):
 *     SEGGER_BCOUNT_ERR_OFFSETS, _CAP, _BUFFER  as SEGGER_PJOIN_ERR_*; such a polygon has an empty row;
 *     SEGGER_BCOUNT_ERR_FILL    the fill found other sizes than indptr and the count call left, or more entries than capacity.
 *
 * Workspace: segger_buffered_counts_workspace_bytes(n_points, n_polygons, n_genes, nx, ny) =
 *   segger_polygon_join_workspace_bytes(n_points, n_polygons, nx, ny) + up(4 N), N = max(n_points, 1), up() rounding up to
 *   256 (n_genes is checked and changes nothing).  256-byte aligned.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: everything segger_polygon_join_* rejects
 *   (n_points and n_polygons below 2^31 - 1), n_genes outside 1 .. SEGGER_BCOUNT_MAX_GENES, a NULL or misaligned gene (4 bytes),
 *   indptr, cell_count, counters (8 bytes), indices or counts (4 bytes).  n_points = 0 or n_polygons = 0 returns SEGGER_OK
 *   without touching a pointer or the device: nothing is written, the caller knows the result is all zeros.
 * ---------------------------------------------------------------------- */
#define SEGGER_BCOUNT_SMALL_GENES 2048
#define SEGGER_BCOUNT_TOUCHED 512
#define SEGGER_BCOUNT_LDS_BYTES 163840
#define SEGGER_BCOUNT_MAX_GENES ((SEGGER_BCOUNT_LDS_BYTES - 65536 - 4 * SEGGER_BCOUNT_TOUCHED) / 4)      /* 24064 */
#define SEGGER_BCOUNT_COUNTERS 5
#define SEGGER_BCOUNT_ERR_OFFSETS 1
#define SEGGER_BCOUNT_ERR_CAP 2
#define SEGGER_BCOUNT_ERR_BUFFER 4
#define SEGGER_BCOUNT_ERR_FILL 8
int64_t segger_buffered_counts_workspace_bytes(int64_t n_points, int64_t n_polygons, int64_t n_genes, int32_t nx, int32_t ny);
int segger_buffered_counts_count(const double* points /* [N, 2] */, int64_t n_points, const int32_t* gene /* [N] */,
                                 int64_t n_genes, const int64_t* ring_offsets, const double* xy, int64_t n_polygons,
                                 int64_t n_vertices, const double* buffer /* [P] fp64 or NULL = 0 */, int32_t predicate,
                                 double x0, double y0, double cell, int32_t nx, int32_t ny, int64_t* indptr /* [P + 1] */,
                                 int64_t* cell_count /* [P] */, int64_t* counters, void* workspace, int64_t workspace_bytes,
                                 segger_stream_t stream);
int segger_buffered_counts_fill(const double* points, int64_t n_points, const int32_t* gene, int64_t n_genes,
                                const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                                const double* buffer, int32_t predicate, double x0, double y0, double cell, int32_t nx,
                                int32_t ny, const int64_t* indptr, const int64_t* cell_count, int32_t* indices, int32_t* counts,
                                int64_t capacity, void* workspace, int64_t workspace_bytes, segger_stream_t stream);

/* ----------------------------------------------------------------------
 * Nearest boundaries (csrc/nearest_boundaries.hip; segger_amd.nearest): for every point the k best of the
 * polygons that segger_polygon_join_* pairs it with, each with its squared distance to the ring and the crossing parity --
 * the two numbers the join's predicate computes and folds into one bit.  A prediction graph with a bounded degree (the
 * reference documents prediction_graph_max_k and ignores it in its shape mode), the signed distance of a transcript to an
 * outline, and erosion as a mask (inside and dist2 >= d d) are read from them.  Purely additive: four new symbols,
 * SEGGER_ABI_VERSION stays 32.
 *
 * Candidates.  The rings, the predicate, the arithmetic, the uniform grid, the walk and its margin are
 *   segger_polygon_join_*'s above: all units compile csrc/ring_predicate.h and csrc/join_grid.h, so the candidates of a point
 *   are the polygons the join lists for it under the same buffer and predicate, bit for bit.
 * Key of a candidate.  parity and dist2 as the join defines them (fp64, coordinates translated to the ring's first vertex,
 *   contraction off);  s = dist2 == 0 ? +0 : (parity ? -dist2 : dist2).  Candidates are ordered by (s, polygon id) ascending:
 *   deeper inside first, then nearer outside; equal s (duplicate polygons, a point on two rings) goes to the lower id.  The
 *   order is strict and total on a point's candidates: a polygon pairs with a point once.
 *
 * Three calls (the number of candidates is known on the device only):
 *   segger_nearest_boundaries_count   bins the points and the polygons as the join does; every match adds one to the
 *       count of its point (an integer atomic); a one-workgroup scan turns the counts into
 *         pair_offsets [n_points + 1] int64   (zeroed by the call), pair_offsets[n_points] = the join's pair total.
 *   segger_nearest_boundaries_fill    the same traversal again, same inputs, the workspace as the count call left it:
 *       a match takes slot pair_offsets[point] + (an integer atomic add on the point's cursor) and writes
 *         pair_key     [capacity] fp64    s;
 *         pair_polygon [capacity] int32   the polygon id, bit 31 set when parity is true (ids are below 2^31 - 1).
 *       Nothing is written at or beyond capacity, nor outside the point's own segment.  The order of a segment's slots
 *       depends on scheduling; nothing that follows depends on it.
 *   segger_nearest_boundaries_select  needs no grid and no workspace.  For point i with c = its candidates, entry j < k:
 *       the smallest (s, id) above entry j - 1 -- k passes over the segment, nothing kept but the last pick: no list in
 *       registers or LDS, no sort.  One lane per point; a point with more than SEGGER_NEAREST_LANE_MAX candidates is
 *       done by its whole wave (lanes stride over the segment, a shuffle reduction takes the minimum).  Writes
 *         polygon_out [n_points, k] int32   the id, n_polygons for j >= c;
 *         dist2_out   [n_points, k] fp64    |s|, +inf for j >= c;
 *         inside_out  [n_points, k] uint8   the parity, 0 for j >= c;
 *         count_out   [n_points]    int32   c, BEFORE the cap k;
 *         counters    [SEGGER_NEAREST_COUNTERS] int64 (zeroed by the call):  0 n_pairs = pair_offsets[n_points];  1 n_kept, the
 *                     sum of min(c, k);  2 n_truncated_points, the points with c > k;  3 max_count.
 *   Integer atomics only, no floating-point accumulation, no scratch; LDS: the 64 KB ring stage of the long-ring route and
 *   nothing else.  Every output is a function of the inputs alone: the same bytes for any grid and any launch geometry.
 *
 * Errors found on the device (the int32 at byte 0 of the workspace, as the join's; the bits are the join's):
 *     SEGGER_NEAREST_ERR_OFFSETS, _CAP, _BUFFER  as SEGGER_PJOIN_ERR_*; such a polygon is nobody's candidate;
 *     SEGGER_NEAREST_ERR_FILL    the fill found more matches of a point than pair_offsets holds, or than capacity.
 *
 * Workspace: segger_nearest_boundaries_workspace_bytes(n_points, n_polygons, nx, ny) =
 *   segger_polygon_join_workspace_bytes(n_points, n_polygons, nx, ny) + up(4 N), N = max(n_points, 1), up() rounding up to
 *   256: the join's layout and an int32 cursor per point.  256-byte aligned.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: everything segger_polygon_join_* rejects, in its
 *   words (count, fill);  k outside 1 .. SEGGER_NEAREST_MAX_K (select);  a negative capacity;  NULL or misaligned pair_key,
 *   dist2_out, counters (8 bytes), pair_polygon, polygon_out, count_out (4 bytes), inside_out.  n_points = 0 or
 *   n_polygons = 0 returns SEGGER_OK from count and fill without touching a pointer or the device; select with n_points = 0
 *   likewise, and with n_polygons = 0 or capacity = 0 (pair_key and pair_polygon may then be NULL) it writes the padding.
 * NOT BUILT: k above SEGGER_NEAREST_MAX_K; holes and multi-part polygons; the eroded geometry as rings (GEOS's buffer(-d));
 *   a scan over more than one workgroup (pair_offsets is scanned by the 1024 threads of counts_to_offsets_kernel).
 * ---------------------------------------------------------------------- */
#define SEGGER_NEAREST_MAX_K 16
#define SEGGER_NEAREST_LANE_MAX 32
#define SEGGER_NEAREST_COUNTERS 4
#define SEGGER_NEAREST_ERR_OFFSETS 1
#define SEGGER_NEAREST_ERR_CAP 2
#define SEGGER_NEAREST_ERR_BUFFER 4
#define SEGGER_NEAREST_ERR_FILL 8
int64_t segger_nearest_boundaries_workspace_bytes(int64_t n_points, int64_t n_polygons, int32_t nx, int32_t ny);
int segger_nearest_boundaries_count(const double* points /* [N, 2] */, int64_t n_points, const int64_t* ring_offsets,
                                    const double* xy, int64_t n_polygons, int64_t n_vertices,
                                    const double* buffer /* [P] fp64 or NULL = 0 */, int32_t predicate, double x0, double y0,
                                    double cell, int32_t nx, int32_t ny, int64_t* pair_offsets /* [N + 1] */, void* workspace,
                                    int64_t workspace_bytes, segger_stream_t stream);
int segger_nearest_boundaries_fill(const double* points, int64_t n_points, const int64_t* ring_offsets, const double* xy,
                                   int64_t n_polygons, int64_t n_vertices, const double* buffer, int32_t predicate, double x0,
                                   double y0, double cell, int32_t nx, int32_t ny, const int64_t* pair_offsets,
                                   double* pair_key, int32_t* pair_polygon, int64_t capacity, void* workspace,
                                   int64_t workspace_bytes, segger_stream_t stream);
int segger_nearest_boundaries_select(const int64_t* pair_offsets, const double* pair_key, const int32_t* pair_polygon,
                                     int64_t capacity, int64_t n_points, int64_t n_polygons, int32_t k, int32_t* polygon_out,
                                     double* dist2_out, uint8_t* inside_out, int32_t* count_out, int64_t* counters,
                                     segger_stream_t stream);

/* ----------------------------------------------------------------------
 * Ring rasterisation (csrc/rasterize.hip; segger_amd.rasterize): an [H, W] int32 label image from a CSR of
 * rings -- the transform opposite to segger_label_contours.  NO REFERENCE COUNTERPART EXISTS (the reference reads label
 * images and never writes one), so the contract below is this project's own; cv2.fillPoly and skimage.draw.polygon follow
 * other pixel rules and could not be run where this was written.  Purely additive: two new symbols, SEGGER_ABI_VERSION
 * stays 32.
 *
 * The rings are segger_polygon_join_*'s: a CSR of single exterior rings in fp64, either orientation, a closing duplicate
 *   dropped, at most SEGGER_MORPH_MAX_VERTS open vertices; a ring of fewer than 3 matches nothing (n_degenerate).
 * The frame is segger_label_contours': the pixel in row r, column c stands for the world point (c sx + tx, r sy + ty) --
 *   one multiplication and one addition in fp64, NOT fused.  sx and sy are finite and non-zero and may be negative.  That
 *   point is tested against the ring as given; the vertices are never transformed back, no division decides anything.
 * The predicate is the join's at distance 0, computed by the same code (csrc/ring_predicate.h: ring_decide(ring_distance(),
 *   0, predicate), the point and the vertices translated to the ring's first vertex, contraction off):
 *     SEGGER_RASTER_INTERSECTS  the closed set: parity or dist2 == 0;     SEGGER_RASTER_CONTAINS  the open set: parity and
 *     dist2 > 0.  The pixels of polygon p are, bit for bit, the pairs segger_polygon_join_* lists for p over the pixel
 *     centres with buffer NULL.  Contour vertices are pixel centres, so INTERSECTS inverts segger_label_contours on a label
 *     of one component without holes.
 * Overlaps.  A pixel matched by several polygons goes to the lowest (SEGGER_RASTER_LOWEST) or the highest
 *   (SEGGER_RASTER_HIGHEST) polygon INDEX -- never the label value: an integer atomic min / max on the index in the image
 *   itself; a finishing pass replaces the index by labels[index] (labels NULL: index + 1; the caller keeps them >= 1) and
 *   writes 0 where nothing matched.  No floating-point atomics, no scratch.  Every output but the two counters marked below
 *   is a function of the inputs alone: the same bytes for any block, either route, any launch geometry and any run.
 * Outputs (all written by the call when n_polygons > 0):
 *     image     [height, width] int32;
 *     n_covered [n_polygons] int64   the pixels of the image the polygon matches, before overlaps are resolved;
 *     n_won     [n_polygons] int64   the pixels that carry the polygon in `image`;
 *     counters  [SEGGER_RASTER_COUNTERS] int64:  0 n_pixels_set;  1 n_overlaps = sum n_covered - n_pixels_set;  2 n_empty,
 *               the polygons with n_covered = 0 (degenerate ones included);  3 n_clipped, the polygons of 3 or more vertices
 *               whose bounds are not inside the closed rectangle of the pixel centres (tx .. (width - 1) sx + tx and the
 *               like in y, computed as the centres are);  4 n_degenerate;  5 n_large_tier, the polygons that ran with the
 *               ring in LDS (ROUTE-DEPENDENT);  6 n_blocks_filled (BLOCK-DEPENDENT).
 * The walk.  One wave per polygon; rings of n <= reg_max (64 or, to force the LDS tier, 0) vertices in registers, the others
 *   in 64 KB of LDS, one single-wave workgroup each, as the join's.  The ring's bounds become a clipped pixel range, widened
 *   by a whole pixel and a rounding margin on every side (csrc/rasterize.hip: pixel_range; the predicate decides membership,
 *   not the range).  The range is taken in block x block pixels (a power of two, 1 .. SEGGER_RASTER_MAX_BLOCK): ring_distance
 *   is evaluated once at the block's centre, and when dist2 exceeds (half_diag (1 + 2^-16) + 2^-30 M)^2 -- half_diag the
 *   distance from the centre to the block's farthest pixel centre, M the magnitude of the coordinates involved; the
 *   argument is written at block_threshold -- no edge passes through the block and all its pixels share the centre's
 *   parity: it is filled or skipped whole.  Other blocks are evaluated pixel by pixel, 64 pixels a step, one per lane.
 *   block = 1 evaluates every pixel of the range.  A large cell costs about area / block^2 + perimeter block evaluations.
 * Errors found on the device (the int32 at byte 0 of the workspace): SEGGER_RASTER_ERR_OFFSETS, _CAP as SEGGER_MORPH_ERR_*;
 *   such a polygon matches nothing.
 * Workspace: segger_rasterize_workspace_bytes(n_polygons) = 256 + 2 up(4 n_polygons), up() rounding up to 256: the words
 *   and one int32 list per route.  256-byte aligned.
 * Rejected on the host with SEGGER_EINVAL and a message, nothing launched: negative sizes, 2^31 - 1 polygons or more, height
 *   or width below 1 or height * width >= 2^31, a zero or non-finite scale, a non-finite translation, an unknown
 *   predicate or overlap, a block that is no power of two in 1 .. SEGGER_RASTER_MAX_BLOCK, reg_max other than 0 or 64, NULL or
 *   misaligned ring_offsets, n_covered, n_won, counters (8 bytes), xy (16), image, labels (4; labels may be NULL), a workspace
 *   that is NULL, misaligned or too small.  n_polygons = 0 returns SEGGER_OK without touching a pointer or the device:
 *   nothing is written, the caller knows the image is all background.
 * NOT BUILT: holes and multi-part polygons; anti-aliased (fractional) coverage; writing TIFF or any file; capture into a
 *   graph; more than one wave per polygon (one huge ring is walked by one wave).
 * ---------------------------------------------------------------------- */
#define SEGGER_RASTER_CONTAINS 0
#define SEGGER_RASTER_INTERSECTS 1
#define SEGGER_RASTER_LOWEST 0
#define SEGGER_RASTER_HIGHEST 1
#define SEGGER_RASTER_MAX_BLOCK 32
#define SEGGER_RASTER_COUNTERS 7
#define SEGGER_RASTER_ERR_OFFSETS 1
#define SEGGER_RASTER_ERR_CAP 2
int64_t segger_rasterize_workspace_bytes(int64_t n_polygons);
int segger_rasterize_rings(const int64_t* ring_offsets, const double* xy, int64_t n_polygons, int64_t n_vertices,
                           const int32_t* labels /* [P] or NULL = index + 1 */, int32_t height, int32_t width, double sx,
                           double sy, double tx, double ty, int32_t predicate, int32_t overlap, int32_t block, int32_t reg_max,
                           int32_t* image /* [H, W] */, int64_t* n_covered /* [P] */, int64_t* n_won /* [P] */,
                           int64_t* counters, void* workspace, int64_t workspace_bytes, segger_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* SEGGER_AMD_H */
