// Host launchers for the fused GATv2 kernels (C ABI: include/segger_amd.h).
#include "gatv2_launch.h"
#include "draws.h"
#include "post_common.h"

namespace segger {

// grad_att / grad_bias = column sums of the slab [nblocks][width], in two deterministic stages:
// stage 1: kSlabSplits row ranges x 64-column chunks -> part[kSlabSplits][width]; stage 2: sum the splits.
// The two-pass backward leaves a second slab [nblocks2][width2] (the source pass's share of grad_att, width2 <= width):
// its columns are summed into the same partials, split into row ranges of its own.
constexpr int kSlabSplits = 128;

__device__ __forceinline__ void slab_stage1_body(const float* __restrict__ slab, int64_t nblocks, int width,
                                                 const float* __restrict__ slab2, int64_t nblocks2, int width2,
                                                 float* __restrict__ part) {
  __shared__ float sm[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int colx = blockIdx.x * 64 + lane;
  const int64_t per = (nblocks + kSlabSplits - 1) / kSlabSplits;
  const int64_t r0 = (int64_t)blockIdx.y * per;
  const int64_t r1 = r0 + per < nblocks ? r0 + per : nblocks;
  float s = 0.f;
  if (colx < width)
    for (int64_t r = r0 + wave; r < r1; r += 4) s += slab[r * width + colx];
  if (colx < width2) {
    const int64_t per2 = (nblocks2 + kSlabSplits - 1) / kSlabSplits;
    const int64_t q0 = (int64_t)blockIdx.y * per2;
    const int64_t q1 = q0 + per2 < nblocks2 ? q0 + per2 : nblocks2;
    // (one slab per 16 source rows: eight times the rows of the first slab, so eight loads in flight per lane)
    float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t r = q0 + wave;
    for (; r + 28 < q1; r += 32) {
#pragma unroll
      for (int k = 0; k < 8; ++k) t[k] += slab2[(r + 4 * k) * width2 + colx];
    }
    for (; r < q1; r += 4) t[0] += slab2[r * width2 + colx];
    s += ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
  }
  sm[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && colx < width) part[(int64_t)blockIdx.y * width + colx] = sm[0][lane] + sm[1][lane] + sm[2][lane] + sm[3][lane];
}

__device__ __forceinline__ void slab_stage2_body(const float* __restrict__ part, int width, int hc,
                                                 float* __restrict__ grad_att, float* __restrict__ grad_bias) {
  const int colx = blockIdx.x * 256 + threadIdx.x;
  if (colx >= width) return;
  float t = 0.f;
  for (int r = 0; r < kSlabSplits; ++r) t += part[(int64_t)r * width + colx];
  if (colx < hc) grad_att[colx] = t;
  else if (grad_bias) grad_bias[colx - hc] = t;
}

__global__ __launch_bounds__(256) void slab_reduce_stage1(const float* __restrict__ slab, int64_t nblocks, int width,
                                                         const float* __restrict__ slab2, int64_t nblocks2, int width2,
                                                         float* __restrict__ part) {
  slab_stage1_body(slab, nblocks, width, slab2, nblocks2, width2, part);
}
__global__ __launch_bounds__(256) void slab_reduce_stage2(const float* __restrict__ part, int width, int hc,
                                                         float* __restrict__ grad_att, float* __restrict__ grad_bias) {
  slab_stage2_body(part, width, hc, grad_att, grad_bias);
}

// The sums of TWO backwards (the edge types of one hetero layer: segger_gatv2_bwd_pair) in one stage-1 / stage-2 pair:
// blockIdx.z picks the job, every job runs the body above on its own slabs and partials -- each sum is the sum, term by
// term and in the same order, that its own launch pair would form.  The grid covers the wider job.
struct SlabJob {
  const float *slab, *slab2; float *part, *grad_att, *grad_bias;
  int64_t nblocks, nblocks2;
  int width, width2, hc;
};
struct SlabJobs { SlabJob job[2]; };

__global__ __launch_bounds__(256) void slab_reduce_stage1_pair(SlabJobs j) {
  const SlabJob& s = j.job[blockIdx.z];
  if ((int)blockIdx.x * 64 >= s.width) return;            // (the whole workgroup: no barrier is left waiting)
  slab_stage1_body(s.slab, s.nblocks, s.width, s.slab2, s.nblocks2, s.width2, s.part);
}
__global__ __launch_bounds__(256) void slab_reduce_stage2_pair(SlabJobs j) {
  const SlabJob& s = j.job[blockIdx.z];
  slab_stage2_body(s.part, s.width, s.hc, s.grad_att, s.grad_bias);
}

// zero the first `pieces` 16-byte pieces of every row of a pitched matrix
__global__ __launch_bounds__(256) void zero_rows_kernel(char* __restrict__ base, int64_t pitch, int64_t pieces, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  *reinterpret_cast<u32x4*>(base + (i / pieces) * pitch + (i % pieces) * 16) = u32x4{0u, 0u, 0u, 0u};
}

__global__ __launch_bounds__(256) void dropout_bits_kernel(BitsParams p) { dropout_bits_body(p, blockIdx.x); }
__global__ __launch_bounds__(256) void dropout_bits_many_kernel(BitsJobs j) { dropout_bits_body(j.job[blockIdx.y], blockIdx.x); }

}  // namespace segger

using namespace segger;

// ---- the host layer: every entry point checks its arguments once into an immutable plan (route flags, workspace carve,
// kernel parameters with their block counts: plan_fwd / plan_bwd), and run_fwd / run_bwd launch what the plan says ------
namespace {

#define CHECK_RC(expr) do { int _rc = (expr); if (_rc != SEGGER_OK) return _rc; } while (0)

// `aligned`: the vectorised (specialised) kernels need 16-byte aligned rows; the generic kernels load element-wise
int check_rows(const char* name, const void* ptr, int64_t ld, int dtype, int hc, bool aligned) {
  SEGGER_REQUIRE(ptr != nullptr, "gatv2: %s is NULL", name);
  SEGGER_REQUIRE(ld >= hc, "gatv2: ld of %s (%lld) < heads*channels (%d)", name, (long long)ld, hc);
  SEGGER_REQUIRE(ld * (int64_t)esize(dtype) < 0xffffffffLL, "gatv2: row stride of %s exceeds 4 GiB", name);
  if (aligned) {
    SEGGER_REQUIRE(is_aligned(ptr, 16), "gatv2: %s is not 16-byte aligned", name);
    SEGGER_REQUIRE((ld * (int64_t)esize(dtype)) % 16 == 0, "gatv2: row stride of %s is not a multiple of 16 bytes", name);
  }
  return SEGGER_OK;
}

int check_csr(const char* name, const segger_csr& g) {
  SEGGER_REQUIRE(g.n_rows >= 0 && g.n_cols >= 0 && g.n_edges >= 0, "gatv2: negative size in %s", name);
  SEGGER_REQUIRE(g.n_rows < 0x7fffffffLL && g.n_cols < 0x7fffffffLL && g.n_edges < 0x7fffffffLL,
                 "gatv2: %s exceeds 2^31-1 rows/cols/edges per batch", name);
  SEGGER_REQUIRE(g.indptr != nullptr, "gatv2: %s.indptr is NULL", name);
  SEGGER_REQUIRE(g.n_edges == 0 || g.col != nullptr, "gatv2: %s.col is NULL", name);
  return SEGGER_OK;
}

// the one refusal of a storage type, ahead of every use of its element size
int check_dtype(int dtype) {
  SEGGER_REQUIRE(dtype == SEGGER_F32 || dtype == SEGGER_BF16 || dtype == SEGGER_F16, "gatv2: unknown dtype %d", dtype);
  return SEGGER_OK;
}

// the block counts of one pass into its parameters (a pair launch adds two of them: still far below 2^31)
int set_grid(GatParams& p, const Grid& g) {
  if (g.nblocks_padded > 0x7fffffffLL) {
    set_error("gatv2: %lld rows need more than 2^31 blocks", (long long)p.n_rows);
    return SEGGER_EUNSUPPORTED;
  }
  p.nblocks = g.nblocks; p.nblocks_padded = g.nblocks_padded;
  return SEGGER_OK;
}

void set_view(GatParams& p, const segger_csr& g) {
  p.indptr = g.indptr; p.col = g.col; p.eid = g.eid; p.order = g.row_order;
  p.n_rows = g.n_rows; p.n_edges = g.n_edges;
}

void set_dropout(GatParams& p, float dropout_p, uint64_t seed, const uint64_t* seed_dev) {
  p.drop_thr = 0; p.drop_scale = 1.f;
  if (dropout_p > 0.f) {
    p.drop_thr = (uint32_t)((double)dropout_p * 16777216.0);
    p.drop_scale = 1.0f / (1.0f - dropout_p);
  }
  const uint64_t mixed = splitmix64(seed);
  p.seed_lo = (uint32_t)(mixed & 0xffffffffu);
  p.seed_hi = (uint32_t)(mixed >> 32);
  p.seed_raw = seed;
  p.seed_dev = seed_dev;
}

// ---- forward ---------------------------------------------------------------------------------------------------
struct GatFwdPlan {
  bool empty = false;                                   // no destination: nothing to launch
  bool specialised = false, wave_per_row = false, alpha = false;
  int dtype = 0, heads = 0, channels = 0;
  GatParams p;
};

int plan_fwd(const segger_gatv2_fwd_args* a, GatFwdPlan& f) {
  SEGGER_REQUIRE(a != nullptr, "segger_gatv2_fwd: args is NULL");
  SEGGER_REQUIRE(a->heads > 0 && a->channels > 0, "segger_gatv2_fwd: heads/channels must be positive");
  CHECK_RC(check_dtype(a->dtype));
  const int hc = a->heads * a->channels;
  const bool spec = gatv2_has_specialised(a->heads, a->channels);
  CHECK_RC(check_csr("by_dst", a->by_dst));
  SEGGER_REQUIRE(a->att != nullptr, "segger_gatv2_fwd: att is NULL");
  SEGGER_REQUIRE(a->negative_slope >= 0.f && a->negative_slope <= 1.f, "segger_gatv2_fwd: negative_slope must be in [0,1]");
  SEGGER_REQUIRE(a->dropout_p >= 0.f && a->dropout_p < 1.f, "segger_gatv2_fwd: dropout_p must be in [0,1)");
  if (a->by_dst.n_rows == 0) { f.empty = true; return SEGGER_OK; }
  CHECK_RC(check_rows("x_r", a->x_r, a->ld_xr, a->dtype, hc, spec));
  CHECK_RC(check_rows("out", a->out, a->ld_out, a->dtype, hc, spec));
  if (a->by_dst.n_edges > 0) CHECK_RC(check_rows("x_l", a->x_l, a->ld_xl, a->dtype, hc, spec));
  if (a->pre) {
    CHECK_RC(check_rows("pre", a->pre, a->ld_pre, a->dtype, hc, spec));
    SEGGER_REQUIRE(!(a->pre == a->out && a->apply_gelu), "segger_gatv2_fwd: pre may alias out only without GELU");
  }
  SEGGER_REQUIRE(!((a->dropout_p > 0.f && !a->keep_bits) || a->alpha) || a->by_dst.n_edges == 0 || a->by_dst.eid != nullptr,
                 "segger_gatv2_fwd: by_dst.eid is required for dropout (without keep_bits) / alpha output");
  f.specialised = spec; f.alpha = a->alpha != nullptr;
  f.wave_per_row = use_wave_per_row(a->by_dst.n_rows, a->by_dst.n_edges);
  f.dtype = a->dtype; f.heads = a->heads; f.channels = a->channels;
  GatParams& p = f.p;
  p = GatParams{};
  set_view(p, a->by_dst);
  if (a->by_dst.blk_cnt && a->by_dst.blk_src && a->by_dst.col_local) {
    p.blk_cnt = a->by_dst.blk_cnt; p.blk_src = a->by_dst.blk_src; p.col_local = a->by_dst.col_local;
  }
  p.xl = a->x_l; p.ld_xl = a->ld_xl; p.xr = a->x_r; p.ld_xr = a->ld_xr;
  p.att = a->att; p.bias = a->bias;
  p.out = a->out; p.ld_out = a->ld_out; p.pre = a->pre; p.ld_pre = a->ld_pre;
  p.lse = a->lse; p.alpha = a->alpha;
  p.bits = a->alpha ? nullptr : a->keep_bits;
  p.slope = a->negative_slope; p.apply_gelu = a->apply_gelu; p.rows_per_wave_iter = 1;
  set_dropout(p, a->dropout_p, a->seed, a->seed_dev);
  return set_grid(p, gatv2_grid(Pass::Fwd, a->heads, a->channels, f.wave_per_row || !spec, 1, p.n_rows));
}

int run_fwd(const GatFwdPlan& f, hipStream_t stream) {
  if (f.empty) return SEGGER_OK;
  if (!f.specialised) return gatv2_launch_generic(Pass::Fwd, f.p, f.dtype, f.heads, f.channels, nullptr, nullptr, stream);
  return launch_specialised(Kind::Fwd, f.dtype, f.p, nullptr, f.heads, f.channels, f.wave_per_row, stream);
}

// ---- backward --------------------------------------------------------------------------------------------------
// workspace of one backward, in floats: [dst_cap][2 HC] destination-pass slab | [src_cap][HC] source-pass slab |
// [kSlabSplits][2 HC] partials of the slab sum.  The capacities are block counts of the grid rule (one slab row per
// block): the destination pass's in the mode with the most blocks, wave-per-row
struct BwdCarve {
  int64_t dst_cap = 0, src_cap = 0;
  float *slab = nullptr, *slab_src = nullptr, *part = nullptr;
  size_t bytes = 0;
};

BwdCarve carve_bwd(void* base, int64_t n_dst, int64_t n_src, int64_t n_edges, int heads, int channels) {
  BwdCarve w;
  const int64_t hc = (int64_t)heads * channels;
  if (n_dst > 0) w.dst_cap = gatv2_grid(Pass::BwdDst, heads, channels, true, bwd_row_iters(n_dst), n_dst).nblocks + kNumXcd;
  if (n_src > 0 && gatv2_has_specialised(heads, channels))
    w.src_cap = gatv2_grid(Pass::BwdSrc, heads, channels, use_wave_per_row(n_src, n_edges), 1, n_src).nblocks + kNumXcd;
  const size_t at_src = (size_t)w.dst_cap * 2 * hc, at_part = at_src + (size_t)w.src_cap * hc;
  w.bytes = (at_part + (size_t)kSlabSplits * 2 * hc) * sizeof(float);
  if (base) { w.slab = static_cast<float*>(base); w.slab_src = w.slab + at_src; w.part = w.slab + at_part; }
  return w;
}

struct GatBwdPlan {
  bool specialised = false, one_pass = false, wpr_dst = false, wpr_src = false;
  bool zero_fill = false;                               // the one-pass form's own zero fill of grad_xl
  int dtype = 0, heads = 0, channels = 0;
  int64_t n_dst = 0, n_src = 0;
  BwdCarve ws;
  float *grad_att = nullptr, *grad_bias = nullptr;
  GatParams dst, src;                                   // the passes' parameters (src: of the two-pass form)
};

// what both passes of a backward read
void bwd_shared(const segger_gatv2_bwd_args* a, const GatBwdPlan& b, GatParams& p) {
  p = GatParams{};
  p.xl = a->x_l; p.ld_xl = a->ld_xl; p.xr = a->x_r; p.ld_xr = a->ld_xr;
  p.att = a->att; p.bias = a->bias;
  p.pre = const_cast<void*>(a->pre); p.ld_pre = a->ld_pre; p.lse = const_cast<float*>(a->lse);
  p.gout = a->grad_out; p.ld_go = a->ld_go; p.gpre = a->grad_pre; p.ld_gp = a->ld_gp; p.dsum = a->dsum;
  p.gxl = a->grad_xl; p.ld_gxl = a->ld_gxl; p.gxr = a->grad_xr; p.ld_gxr = a->ld_gxr;
  p.slab = b.ws.slab; p.slab_src = b.ws.slab_src;
  p.slope = a->negative_slope; p.apply_gelu = a->apply_gelu;
  set_dropout(p, a->dropout_p, a->seed, a->seed_dev);
}

// parameters of the destination-side pass (rows = destinations); `zero`: a matrix of one row per destination it
// zero-fills on its way, or NULL.  The generic kernel walks one row batch per wave whatever rows_per_wave_iter says
int dst_pass(const segger_gatv2_bwd_args* a, const GatBwdPlan& b, void* zero, int64_t ld_zero, GatParams& p) {
  bwd_shared(a, b, p);
  set_view(p, a->by_dst);
  p.bits = a->keep_bits_dst;
  p.rows_per_wave_iter = bwd_row_iters(b.n_dst);
  p.direct_gxl = b.one_pass ? 1 : 0;
  p.zero_rows = zero; p.ld_zero = ld_zero;
  CHECK_RC(set_grid(p, gatv2_grid(Pass::BwdDst, b.heads, b.channels, b.wpr_dst || !b.specialised,
                                  b.specialised ? p.rows_per_wave_iter : 1, p.n_rows)));
  SEGGER_REQUIRE(!b.specialised || p.nblocks <= b.ws.dst_cap, "segger_gatv2_bwd: the destination pass's blocks exceed its slab");
  return SEGGER_OK;
}

// parameters of the source-side pass (rows = sources); `zero`: a matrix of one row per source it zero-fills, or NULL
int src_pass(const segger_gatv2_bwd_args* a, const GatBwdPlan& b, void* zero, int64_t ld_zero, GatParams& p) {
  bwd_shared(a, b, p);
  set_view(p, a->by_src);
  p.bits = a->keep_bits_src;
  p.rows_per_wave_iter = 1;
  p.zero_rows = zero; p.ld_zero = ld_zero;
  CHECK_RC(set_grid(p, gatv2_grid(Pass::BwdSrc, b.heads, b.channels, b.wpr_src || !b.specialised, 1, p.n_rows)));
  SEGGER_REQUIRE(!b.specialised || p.nblocks <= b.ws.src_cap, "segger_gatv2_bwd: the source pass's blocks exceed its slab");
  return SEGGER_OK;
}

int plan_bwd(const segger_gatv2_bwd_args* a, GatBwdPlan& b) {
  SEGGER_REQUIRE(a != nullptr, "segger_gatv2_bwd: args is NULL");
  SEGGER_REQUIRE(a->heads > 0 && a->channels > 0, "segger_gatv2_bwd: heads/channels must be positive");
  CHECK_RC(check_dtype(a->dtype));
  const int hc = a->heads * a->channels;
  const bool spec = gatv2_has_specialised(a->heads, a->channels);
  CHECK_RC(check_csr("by_dst", a->by_dst));
  const bool direct = a->src_unique != 0;
  SEGGER_REQUIRE(!direct || spec, "segger_gatv2_bwd: src_unique needs a specialised (heads, channels) geometry");
  if (!direct) {
    CHECK_RC(check_csr("by_src", a->by_src));
    SEGGER_REQUIRE(a->by_dst.n_edges == a->by_src.n_edges && a->by_dst.n_rows == a->by_src.n_cols &&
                   a->by_dst.n_cols == a->by_src.n_rows, "segger_gatv2_bwd: by_dst and by_src describe different graphs");
  }
  SEGGER_REQUIRE(a->att && a->grad_att, "segger_gatv2_bwd: att / grad_att is NULL");
  SEGGER_REQUIRE(a->negative_slope >= 0.f && a->negative_slope <= 1.f, "segger_gatv2_bwd: negative_slope must be in [0,1]");
  SEGGER_REQUIRE(a->dropout_p >= 0.f && a->dropout_p < 1.f, "segger_gatv2_bwd: dropout_p must be in [0,1)");
  const int64_t n_dst = a->by_dst.n_rows, n_src = a->by_dst.n_cols, n_edges = a->by_dst.n_edges;
  if (n_dst > 0) {
    CHECK_RC(check_rows("x_r", a->x_r, a->ld_xr, a->dtype, hc, spec));
    CHECK_RC(check_rows("grad_out", a->grad_out, a->ld_go, a->dtype, hc, spec));
    CHECK_RC(check_rows("pre", a->pre, a->ld_pre, a->dtype, hc, spec));
    CHECK_RC(check_rows("grad_pre", a->grad_pre, a->ld_gp, a->dtype, hc, spec));
    CHECK_RC(check_rows("grad_xr", a->grad_xr, a->ld_gxr, a->dtype, hc, spec));
    SEGGER_REQUIRE(a->lse && a->dsum, "segger_gatv2_bwd: lse / dsum is NULL");
  }
  if (n_src > 0) {
    CHECK_RC(check_rows("x_l", a->x_l, a->ld_xl, a->dtype, hc, spec));
    CHECK_RC(check_rows("grad_xl", a->grad_xl, a->ld_gxl, a->dtype, hc, spec));
  }
  SEGGER_REQUIRE(!(a->dropout_p > 0.f) || n_edges == 0 ||
                     ((a->by_dst.eid || a->keep_bits_dst) && (direct || a->by_src.eid || a->keep_bits_src)),
                 "segger_gatv2_bwd: eid arrays (or keep_bits) are required for dropout");
  b.ws = carve_bwd(a->workspace, n_dst, direct ? 0 : n_src, direct ? 0 : n_edges, a->heads, a->channels);
  const size_t need = (n_dst > 0 || b.ws.src_cap > 0) ? b.ws.bytes : 16;
  if (a->workspace == nullptr || a->workspace_bytes < need) {
    set_error("segger_gatv2_bwd: workspace %zu < %zu bytes", a->workspace_bytes, need);
    return SEGGER_EWORKSPACE;
  }
  SEGGER_REQUIRE(!a->zero_rows_out || (!direct && spec),
                 "segger_gatv2_bwd: zero_rows_out needs the two-pass backward of a specialised geometry");
  if (a->zero_rows_out && n_src > 0) CHECK_RC(check_rows("zero_rows_out", a->zero_rows_out, a->ld_zero, a->dtype, hc, spec));

  b.specialised = spec; b.one_pass = direct;
  b.wpr_dst = use_wave_per_row(n_dst, n_edges);
  b.wpr_src = !direct && use_wave_per_row(n_src, n_edges);
  b.zero_fill = direct && n_src > 0 && !a->grad_xl_zeroed;
  b.dtype = a->dtype; b.heads = a->heads; b.channels = a->channels;
  b.n_dst = n_dst; b.n_src = n_src;
  b.grad_att = a->grad_att; b.grad_bias = a->grad_bias;
  CHECK_RC(dst_pass(a, b, nullptr, 0, b.dst));
  if (!direct) CHECK_RC(src_pass(a, b, a->zero_rows_out, a->ld_zero, b.src));
  return SEGGER_OK;
}

int launch_pass(Pass pass, const GatBwdPlan& b, const GatParams& p, bool wave_per_row, hipStream_t stream) {
  if (!b.specialised) return gatv2_launch_generic(pass, p, b.dtype, b.heads, b.channels, b.grad_att, b.grad_bias, stream);
  return launch_specialised((Kind)pass, b.dtype, p, nullptr, b.heads, b.channels, wave_per_row, stream);
}

// the one-pass form's own zero fill: sources without an out-edge keep a zero gradient, the others are stored by the
// destination pass (rows are 16-byte aligned multiples of 16 bytes: checked by the plan.  hipMemset2DAsync measured
// 0.19 ms for 1M x 256 B at pitch 768; this kernel 0.05 ms)
int bwd_zero_fill(const GatBwdPlan& b, hipStream_t stream) {
  const size_t es = esize(b.dtype);
  const int64_t pieces = (int64_t)b.heads * b.channels * es / 16, total = b.n_src * pieces;
  hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                     static_cast<char*>(b.dst.gxl), b.dst.ld_gxl * (int64_t)es, pieces, total);
  SEGGER_LAUNCH_CHECK("zero_rows_kernel");
  return SEGGER_OK;
}

// grad_att / grad_bias from the per-block slabs the passes left behind: dst_blocks rows of the destination pass and,
// after a source pass, src_blocks rows of grad_att alone
ReduceSeg slab_seg(const GatBwdPlan& b, int64_t dst_blocks, int64_t src_blocks) {
  const int hc = b.heads * b.channels;
  return ReduceSeg{b.ws.slab, dst_blocks, 2 * hc, hc, b.grad_att, b.grad_bias, b.ws.part, b.ws.slab_src,
                   (int32_t)src_blocks, src_blocks > 0 ? hc : 0};
}

int bwd_reduce_slab(const GatBwdPlan& b, int64_t dst_blocks, int64_t src_blocks, hipStream_t stream) {
  if (!b.specialised) return SEGGER_OK;                   // the generic kernels write grad_att / grad_bias themselves
  const int hc = b.heads * b.channels, width = 2 * hc;
  const int width2 = src_blocks > 0 ? hc : 0;
  if (defer_reduce(slab_seg(b, dst_blocks, src_blocks), stream)) return SEGGER_OK;
  hipLaunchKernelGGL(slab_reduce_stage1, dim3((width + 63) / 64, kSlabSplits), dim3(256), 0, stream,
                     b.ws.slab, dst_blocks, width, b.ws.slab_src, src_blocks, width2, b.ws.part);
  hipLaunchKernelGGL(slab_reduce_stage2, dim3((width + 255) / 256), dim3(256), 0, stream,
                     b.ws.part, width, hc, b.grad_att, b.grad_bias);
  SEGGER_LAUNCH_CHECK("slab_reduce kernels");
  return SEGGER_OK;
}

// The two sums of a merged backward pair (`a`: both passes' slabs, `b`: the one-pass form's) in one launch pair instead of
// two.  With the partial-sum queue of reduce.hip active (captured steps) both go to it, as they do one by one.
int bwd_reduce_slab_pair(const GatBwdPlan& a, int64_t a_dst_blocks, int64_t a_src_blocks, const GatBwdPlan& b,
                         int64_t b_dst_blocks, hipStream_t stream) {
  const int hc_a = a.heads * a.channels, hc_b = b.heads * b.channels;
  if (defer_reduce(slab_seg(a, a_dst_blocks, a_src_blocks), stream)) return bwd_reduce_slab(b, b_dst_blocks, 0, stream);
  SlabJobs j{};
  j.job[0] = SlabJob{a.ws.slab, a.ws.slab_src, a.ws.part, a.grad_att, a.grad_bias, a_dst_blocks, a_src_blocks,
                     2 * hc_a, a_src_blocks > 0 ? hc_a : 0, hc_a};
  j.job[1] = SlabJob{b.ws.slab, nullptr, b.ws.part, b.grad_att, b.grad_bias, b_dst_blocks, 0, 2 * hc_b, 0, hc_b};
  const int width = 2 * (hc_a > hc_b ? hc_a : hc_b);
  hipLaunchKernelGGL(slab_reduce_stage1_pair, dim3((width + 63) / 64, kSlabSplits, 2), dim3(256), 0, stream, j);
  hipLaunchKernelGGL(slab_reduce_stage2_pair, dim3((width + 255) / 256, 1, 2), dim3(256), 0, stream, j);
  SEGGER_LAUNCH_CHECK("slab_reduce pair kernels");
  return SEGGER_OK;
}

// SEGGER_BWD_ONE_PASS_IN_PAIR_KERNEL=1 (read once): segger_gatv2_bwd runs the wave-per-row one-pass form as the merged
// kernel of segger_gatv2_bwd_pair with an EMPTY source-pass side instead of as gatv2_bwd_dst_kernel -- the merged launch's
// tx-belongs-bd body by itself, for bit comparisons against the merged launch and for timing.  Results agree with the
// default kernel to rounding (another number of rows in flight, the lean grad_att form).
bool bwd_one_pass_in_pair_kernel() {
  static const bool v = [] { const char* e = getenv("SEGGER_BWD_ONE_PASS_IN_PAIR_KERNEL"); return e && atoi(e) != 0; }();
  return v;
}

// passes: 0 both, 1 the destination pass with its sums, 2 the source pass alone, 3 the destination pass without sums
int run_bwd(const GatBwdPlan& b, int passes, hipStream_t stream) {
  SEGGER_REQUIRE(passes >= 0 && passes <= 3, "segger_gatv2_bwd: passes must be 0 (both), 1 (destination), 2 (source) or 3");
  if (passes != 2) {
    if (b.zero_fill) CHECK_RC(bwd_zero_fill(b, stream));
    if (b.n_dst > 0) {
      if (b.one_pass && b.specialised && b.wpr_dst && bwd_one_pass_in_pair_kernel()) {
        const GatParams none{};                            // (no block of the source pass: its parameters are never read)
        CHECK_RC(launch_specialised(Kind::BwdSrcDstPair, b.dtype, none, &b.dst, b.heads, b.channels, false, stream));
      } else {
        CHECK_RC(launch_pass(Pass::BwdDst, b, b.dst, b.wpr_dst, stream));
      }
      // the one-pass form and passes = 1 end here: the sums of the destination pass alone
      if (b.one_pass || passes == 1) CHECK_RC(bwd_reduce_slab(b, b.dst.nblocks, 0, stream));
    } else {                                                // no destination: the sums are zero
      SEGGER_HIP(hipMemsetAsync(b.grad_att, 0, b.heads * b.channels * sizeof(float), stream));
      if (b.grad_bias) SEGGER_HIP(hipMemsetAsync(b.grad_bias, 0, b.heads * b.channels * sizeof(float), stream));
    }
  }
  if (b.one_pass || passes == 1 || passes == 3) return SEGGER_OK;
  if (b.n_src > 0) CHECK_RC(launch_pass(Pass::BwdSrc, b, b.src, b.wpr_src, stream));
  // grad_att needs both passes' slabs: summed once, behind the source pass (passes = 2 is the source kernel alone)
  if (passes == 0 && b.n_dst > 0) CHECK_RC(bwd_reduce_slab(b, b.dst.nblocks, b.n_src > 0 ? b.src.nblocks : 0, stream));
  return SEGGER_OK;
}

// largest tx-neighbors-tx source count for which segger_gatv2_bwd_pair merges the launches: every size unless the
// environment says otherwise.  What the merger saves is the one-pass launch, latency-bound at every size (~5 us per layer
// on the captured 1M-edge step, 68 us per layer on the C2 tile), and one slab-sum launch pair.
// SEGGER_BWD_PAIR_MAX_ROWS=262144 restores the route rule of the builds before the merged kernel kept the source pass's
// occupancy (separate launches above that size), =0 separate launches at every size: both routes from one build.
int64_t bwd_pair_max_rows() {
  static const int64_t v = [] {
    const char* e = getenv("SEGGER_BWD_PAIR_MAX_ROWS");
    return e ? (int64_t)atoll(e) : (int64_t)SEGGER_BWD_PAIR_MAX_ROWS;
  }();
  return v;
}

// checks + fields of one bit-plane job in the name of entry point `who`; job < 0: its only one
int fill_bits(const char* who, int job, const segger_bits_job& jb, int heads, float dropout_p, const uint64_t* seed_dev,
              BitsParams* out) {
  const auto refuse = [&](const char* what) {
    if (job < 0) set_error("%s: %s", who, what); else set_error("%s: job %d: %s", who, job, what);
    return SEGGER_EINVAL;
  };
  if (!(jb.n_edges >= 0 && jb.n_seeds > 0 && jb.n_seeds <= 16)) return refuse("bad sizes");
  if (!(jb.n_edges == 0 || (jb.eid && jb.bits))) return refuse("NULL pointer");
  if (!(jb.plane_stride >= jb.n_edges && jb.plane_stride % 4 == 0 && ((uintptr_t)jb.bits & 3u) == 0))
    return refuse("plane_stride must be a multiple of 4 >= n_edges, bits 4-byte aligned");
  BitsParams& p = *out;
  p = BitsParams{};
  p.eid = jb.eid; p.n_edges = jb.n_edges; p.plane_stride = jb.plane_stride; p.heads = heads; p.n_seeds = jb.n_seeds;
  p.seed_dev = seed_dev; p.bits = jb.bits; p.eid_aligned = is_aligned(jb.eid, 16) ? 1 : 0;
  p.thr = (uint32_t)((double)dropout_p * 16777216.0);
  for (int l = 0; l < jb.n_seeds; ++l) p.seeds[l] = jb.seeds[l];
  return SEGGER_OK;
}

}  // namespace

extern "C" int segger_gatv2_fwd(const segger_gatv2_fwd_args* a, segger_stream_t stream) {
  GatFwdPlan f;
  CHECK_RC(plan_fwd(a, f));
  return run_fwd(f, (hipStream_t)stream);
}

extern "C" int segger_gatv2_fwd_pair(const segger_gatv2_fwd_args* a, const segger_gatv2_fwd_args* b, segger_stream_t stream) {
  GatFwdPlan fa, fb;
  CHECK_RC(plan_fwd(a, fa));
  CHECK_RC(plan_fwd(b, fb));
  // one launch when `a` is a low-degree (group-per-row) and `b` a high-degree (wave-per-row) edge type of the same
  // specialised geometry and storage type and neither asks for attention weights; otherwise two launches
  const bool one = !fa.empty && !fb.empty && fa.dtype == fb.dtype && fa.heads == fb.heads && fa.channels == fb.channels &&
                   fa.specialised && !fa.wave_per_row && fb.wave_per_row && !fa.alpha && !fb.alpha;
  if (one) return launch_specialised(Kind::FwdPair, fa.dtype, fa.p, &fb.p, fa.heads, fa.channels, false, (hipStream_t)stream);
  CHECK_RC(run_fwd(fa, (hipStream_t)stream));
  return run_fwd(fb, (hipStream_t)stream);
}

extern "C" size_t segger_gatv2_bwd_workspace_bytes_two_pass(int64_t n_dst, int64_t n_src, int64_t n_edges, int32_t heads,
                                                           int32_t channels) {
  if ((n_dst <= 0 && n_src <= 0) || heads <= 0 || channels <= 0) return 16;
  return carve_bwd(nullptr, n_dst, n_src, n_edges, heads, channels).bytes;
}

extern "C" size_t segger_gatv2_bwd_workspace_bytes(int64_t n_dst, int32_t heads, int32_t channels) {
  return segger_gatv2_bwd_workspace_bytes_two_pass(n_dst, 0, 0, heads, channels);
}

extern "C" int segger_gatv2_bwd(const segger_gatv2_bwd_args* a, segger_stream_t stream) {
  GatBwdPlan b;
  CHECK_RC(plan_bwd(a, b));
  return run_bwd(b, a->passes, (hipStream_t)stream);
}

extern "C" int segger_gatv2_bwd_pair(const segger_gatv2_bwd_args* a, const segger_gatv2_bwd_args* b, segger_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  GatBwdPlan pa, pb;
  CHECK_RC(plan_bwd(a, pa));
  CHECK_RC(plan_bwd(b, pb));
  // one launch for a's source pass and b's one-pass destination pass when: a is a two-pass, group-per-row edge type
  // and b a one-pass, wave-per-row one of the same specialised geometry and storage type; both non-empty; b's grad_xl
  // is the matrix a was asked to zero-fill (or a was asked for none and b's is not zeroed yet) and a's destinations
  // index the same nodes as b's sources -- a's DESTINATION pass then zero-fills it, since its source pass now runs
  // beside b's stores; and the route switch allows the size (bwd_pair_max_rows: every size by default)
  const bool zero_by_a = a->zero_rows_out ? (a->zero_rows_out == b->grad_xl && a->ld_zero == b->ld_gxl && b->grad_xl_zeroed)
                                          : !b->grad_xl_zeroed;
  const bool one = !pa.one_pass && pb.one_pass && pa.dtype == pb.dtype && pa.heads == pb.heads && pa.channels == pb.channels &&
                   pa.specialised && pa.n_dst > 0 && pa.n_src > 0 && pb.n_dst > 0 && pb.n_src > 0 && pa.n_dst == pb.n_src &&
                   !pa.wpr_dst && !pa.wpr_src && pb.wpr_dst && zero_by_a && pa.n_src <= bwd_pair_max_rows();
  if (!one) {
    CHECK_RC(run_bwd(pa, a->passes, stream));
    return run_bwd(pb, b->passes, stream);
  }
  // the merged route has passes of its own: a's destination pass zero-fills b's grad_xl, a's source pass nothing
  GatParams a_dst, a_src;
  CHECK_RC(dst_pass(a, pa, b->grad_xl, b->ld_gxl, a_dst));
  CHECK_RC(src_pass(a, pa, nullptr, 0, a_src));
  CHECK_RC(launch_pass(Pass::BwdDst, pa, a_dst, false, stream));
  CHECK_RC(launch_specialised(Kind::BwdSrcDstPair, pa.dtype, a_src, &pb.dst, pa.heads, pa.channels, false, stream));
  return bwd_reduce_slab_pair(pa, a_dst.nblocks, a_src.nblocks, pb, pb.dst.nblocks, stream);
}

extern "C" int segger_gatv2_has_specialised(int32_t heads, int32_t channels) {
  return gatv2_has_specialised(heads, channels) ? 1 : 0;
}

extern "C" int segger_dropout_bits(const int32_t* eid, int64_t n_edges, int32_t heads, float dropout_p,
                                   const uint64_t* seeds, int32_t n_seeds, const uint64_t* seed_dev, uint8_t* bits,
                                   int64_t plane_stride, segger_stream_t stream) {
  SEGGER_REQUIRE(n_edges >= 0 && heads > 0 && heads <= 8, "segger_dropout_bits: heads must be in 1..8");
  SEGGER_REQUIRE(n_seeds > 0 && n_seeds <= 16 && seeds, "segger_dropout_bits: 1..16 seeds");
  SEGGER_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "segger_dropout_bits: dropout_p must be in [0,1)");
  if (n_edges == 0) return SEGGER_OK;
  segger_bits_job jb{};
  jb.eid = eid; jb.n_edges = n_edges; jb.seeds = seeds; jb.n_seeds = n_seeds; jb.bits = bits; jb.plane_stride = plane_stride;
  BitsParams p;
  CHECK_RC(fill_bits("segger_dropout_bits", -1, jb, heads, dropout_p, seed_dev, &p));
  hipLaunchKernelGGL(dropout_bits_kernel, dim3((unsigned)((n_edges + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, p);
  SEGGER_LAUNCH_CHECK("dropout_bits_kernel");
  return SEGGER_OK;
}

namespace segger {
// (declared in draws.h for the step's draw launch, which reports in this entry point's name)
int fill_bits_params(const segger_bits_job& jb, int heads, float dropout_p, const uint64_t* seed_dev, int i, BitsParams* out) {
  return fill_bits("segger_dropout_bits_many", i, jb, heads, dropout_p, seed_dev, out);
}
}  // namespace segger

extern "C" int segger_dropout_bits_many(const segger_bits_job* jobs, int32_t n_jobs, int32_t heads, float dropout_p,
                                        const uint64_t* seed_dev, segger_stream_t stream) {
  SEGGER_REQUIRE(jobs && n_jobs > 0 && n_jobs <= kMaxBitsJobs, "segger_dropout_bits_many: 1..4 jobs");
  SEGGER_REQUIRE(heads > 0 && heads <= 8, "segger_dropout_bits_many: heads must be in 1..8");
  SEGGER_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "segger_dropout_bits_many: dropout_p must be in [0,1)");
  BitsJobs all{};
  int64_t most = 0;
  for (int i = 0; i < n_jobs; ++i) {
    CHECK_RC(fill_bits_params(jobs[i], heads, dropout_p, seed_dev, i, &all.job[i]));
    if (jobs[i].n_edges > most) most = jobs[i].n_edges;
  }
  if (most == 0) return SEGGER_OK;
  hipLaunchKernelGGL(dropout_bits_many_kernel, dim3((unsigned)((most + 1023) / 1024), (unsigned)n_jobs), dim3(256), 0,
                     (hipStream_t)stream, all);
  SEGGER_LAUNCH_CHECK("dropout_bits_many_kernel");
  return SEGGER_OK;
}

namespace segger {
namespace {
__global__ void step_advance_kernel(int64_t* step, int64_t inc, int64_t* copy) {
  if (threadIdx.x == 0) { const int64_t v = *step + inc; *step = v; if (copy) *copy = v; }
}
}  // namespace
}  // namespace segger

extern "C" int segger_step_advance(int64_t* step, int64_t inc, int64_t* copy, segger_stream_t stream) {
  SEGGER_REQUIRE(step != nullptr, "segger_step_advance: step is NULL");
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step, inc, copy);
  SEGGER_LAUNCH_CHECK("step_advance_kernel");
  return SEGGER_OK;
}
