// Tall-skinny projection GEMM on the matrix cores:  Y[n, M] = X[n, K] * W[M, K]^T (+ bias)
// for n ~ 10^6 node rows and small K, M (<= 384): the lin_l / lin_r / lin_last maps
// of the encoder and their data-gradients (dX = dY * W, called with W^T).
//
// The op is HBM-bound (2*n*(K+M) bytes against 2*n*K*M flops at K,M <= 384), so the
// design goal is "read X once, write Y once":
//   * one workgroup (4 waves) owns 128 consecutive rows and produces ALL M columns,
//     so X is never re-read per column tile;
//   * a wave keeps its 32 rows of X as MFMA B-operand fragments in registers for
//     the whole block (K/16 x 4 VGPRs), loaded straight from global memory;
//   * W is streamed through LDS in chunks of 64 output columns shared by the 4
//     waves (row stride K*2+16 B: conflict-free ds_read_b128 of A fragments), with
//     the next chunk prefetched into registers under the MFMAs;
//   * D = W_tile * X_tile^T  (v_mfma_f32_32x32x16, mma.h's Mfma<T>::run): a lane owns one DATA ROW and
//     4-column groups, so the epilogue packs 4 bf16 -> ds_write_b64 into a wave-private
//     LDS tile and streams it out as full 128-byte row segments (16 B per lane).
#include <algorithm>
#include "common.h"
#include "mma.h"
#include "post_common.h"

namespace segger {
namespace {

constexpr int kRowsPerBlock = 128;
constexpr int kChunk = 64;             // output columns per W chunk

struct LinearParams {
  const void* x; int64_t ldx;
  const void* w;            // [m_out, K] row-major, same dtype as x
  const float* bias;        // [m_out] or NULL
  void* y; int64_t ldy;
  int64_t n_rows;
  int m_out;
  // optional per-row additive term: y[row, :] += rowbias[rowidx[row], :] (fp32 table, row stride ld_rb elements) -- the
  // part of a projection that depends on a row only through a small categorical id (ist_encoder's gene embedding)
  const void* rowbias; const int32_t* rowidx; int64_t ld_rb;      // (table in the activation dtype)
  // optional epilogue factor: y[row, c] *= silu'(gate[row, c]) (gate in the activation dtype, row stride ld_gate) -- the
  // backward of Linear -> SiLU without a separate elementwise pass over dX
  const void* gate; int64_t ld_gate;
};

template <int K> constexpr int linear_lds_bytes() { return kChunk * (K * 2 + 16) + 4 * 32 * (kChunk * 2 + 16); }

// `lds`: the workgroup's shared array of linear_lds_bytes<K>() bytes (declared by the kernel: two bodies of a pair launch
// share one array instead of adding theirs up)
template <typename T, int K, bool RB = false, bool SG = false>
__device__ __forceinline__ void linear_fwd_body(const LinearParams p, const int64_t bid, unsigned char* lds) {
  constexpr int NK = K / 16;                       // k-steps
  constexpr int WSTRIDE = K * 2 + 16;              // bytes per LDS row of W
  constexpr int ESTRIDE = kChunk * 2 + 16;         // bytes per LDS row of the epilogue tile
  constexpr int PIECES = kChunk * K * 2 / 16;      // 16-byte pieces per W chunk
  constexpr int PPT = PIECES / 256;                // pieces per thread
  static_assert(PIECES % 256 == 0, "chunk must split evenly over the block");
  unsigned char* lds_w = lds;
  unsigned char* lds_e = lds + kChunk * WSTRIDE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t row0 = bid * kRowsPerBlock + wave * 32;
  const T* __restrict__ x = static_cast<const T*>(p.x);
  const T* __restrict__ w = static_cast<const T*>(p.w);
  T* __restrict__ y = static_cast<T*>(p.y);

  // ---- X fragments: lane (r,h) holds X[row0+r][16s+8h .. +8) for every k-step s -----------------
  u32x4 xb[NK];
  {
    int64_t row = row0 + r;
    if (row >= p.n_rows) row = p.n_rows - 1;       // clamp: loaded, never stored
    const T* xr = x + row * p.ldx + 8 * h;
#pragma unroll
    for (int s = 0; s < NK; ++s) xb[s] = *reinterpret_cast<const u32x4*>(xr + 16 * s);
  }

  // ---- W chunk staging ------------------------------------------------------------------------------
  u32x4 wreg[PPT];
  auto w_fetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int piece = tid + 256 * i;
      const int wrow = piece / (K / 8), wcol = piece % (K / 8);
      wreg[i] = *reinterpret_cast<const u32x4*>(w + (int64_t)(c0 + wrow) * K + wcol * 8);
    }
  };
  auto w_commit = [&]() {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int piece = tid + 256 * i;
      const int wrow = piece / (K / 8), wcol = piece % (K / 8);
      *reinterpret_cast<u32x4*>(lds_w + wrow * WSTRIDE + wcol * 16) = wreg[i];
    }
  };

  const int n_chunks = p.m_out / kChunk;
  // per-row additive table row of this lane's data row (its columns are fetched per chunk, ahead of the MFMAs)
  const T* gate_row = nullptr;
  // RB: the table rows of this wave's 32 data rows are fetched as whole 128-byte chunk segments -- lane (8 i + lane / 8,
  // piece lane % 8) loads 16 bytes, 8 rows x 128 B per instruction -- and handed to the lanes that own the output
  // columns through the wave's epilogue tile.  (Round 2 let every lane fetch its own 8-byte column groups: 32 table
  // rows x 16 B per instruction, twice the instructions and four times the cache lines per instruction: 0.31 ms for
  // the first layer against 0.22 ms for the plain projection.)
  const T* rb_rows[4] = {nullptr, nullptr, nullptr, nullptr};
  if (RB) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t row = row0 + 8 * i + (lane >> 3);
      if (row >= p.n_rows) row = p.n_rows - 1;
      rb_rows[i] = static_cast<const T*>(p.rowbias) + (int64_t)p.rowidx[row] * p.ld_rb + 8 * (lane & 7);
    }
  }
  if (SG) {
    int64_t row = row0 + r;
    if (row >= p.n_rows) row = p.n_rows - 1;
    gate_row = static_cast<const T*>(p.gate) + row * p.ld_gate + 4 * h;
  }
  w_fetch(0);
  for (int c = 0; c < n_chunks; ++c) {
    const int c0 = c * kChunk;
    w_commit();                                    // all waves left the previous chunk's MFMA loop (epilogue barrier)
    __syncthreads();
    if (c + 1 < n_chunks) w_fetch(c0 + kChunk);    // prefetch under the MFMAs
    // this lane's 4-column groups of the table row / the gate row, requested ahead of the MFMAs
    uint2 rbv[SG ? 2 : 1][SG ? 4 : 1];
    u32x4 rbq[RB ? 4 : 1];
    if (SG) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) rbv[ct][g] = *reinterpret_cast<const uint2*>(gate_row + c0 + ct * 32 + 8 * g);
    }
    if (RB) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rbq[i] = *reinterpret_cast<const u32x4*>(rb_rows[i] + c0);
    }

    f32x16 acc[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < NK; ++s) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(lds_w + (ct * 32 + r) * WSTRIDE + (16 * s + 8 * h) * 2);
        acc[ct] = Mfma<T>::run(a, xb[s], acc[ct]);
      }
    }

    // ---- epilogue: lane owns data row r and output columns ct*32 + 8g + 4h + {0..3} -------------
    unsigned char* et = lds_e + wave * 32 * ESTRIDE;
    if (RB) {
      // table segments -> the wave's tile (same layout as the output tile); every lane then reads its own column
      // groups back and overwrites exactly those bytes with the result: LDS operations of one wave execute in order
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<u32x4*>(et + (8 * i + (lane >> 3)) * ESTRIDE + (lane & 7) * 16) = rbq[i];
    }

#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = ct * 32 + 8 * g + 4 * h;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[ct][4 * g + j] + (p.bias ? p.bias[c0 + col + j] : 0.f);
        if (RB) {
          const uint2 tt = *reinterpret_cast<const uint2*>(et + r * ESTRIDE + col * 2);
          float t4[4];
          Vec8<T>::unpack2(tt.x, t4[0], t4[1]);
          Vec8<T>::unpack2(tt.y, t4[2], t4[3]);
          v[0] += t4[0]; v[1] += t4[1]; v[2] += t4[2]; v[3] += t4[3];
        }
        if (SG) {
          const uint2 zz = rbv[SG ? ct : 0][SG ? g : 0];
          float z[4];
          Vec8<T>::unpack2(zz.x, z[0], z[1]);
          Vec8<T>::unpack2(zz.y, z[2], z[3]);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= silu_grad(z[j]);
        }
        uint2 pk;
        pk.x = Vec8<T>::pack(v[0], v[1]);
        pk.y = Vec8<T>::pack(v[2], v[3]);
        *reinterpret_cast<uint2*>(et + r * ESTRIDE + col * 2) = pk;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int er = 8 * i + (lane >> 3), piece = lane & 7;
      const u32x4 v = *reinterpret_cast<const u32x4*>(et + er * ESTRIDE + piece * 16);
      const int64_t row = row0 + er;
      if (row < p.n_rows) *reinterpret_cast<u32x4*>(y + row * p.ldy + c0 + piece * 8) = v;
    }
  }
}

template <typename T, int K, bool RB = false, bool SG = false>
__global__ __launch_bounds__(256, 2) void linear_fwd_kernel(LinearParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[linear_lds_bytes<K>()];
  linear_fwd_body<T, K, RB, SG>(p, blockIdx.x, lds);
}

// Two projections with the same K in ONE launch: the blocks of `b` (a few: the boundary side of a hetero layer, ~500 rows)
// are dispatched first and run beside the blocks of `a` instead of as a 7 us launch of their own (a captured 1M-edge
// training step has six such pairs; same idea as gatv2_fwd_pair_kernel).
template <typename T, int KA, int KB = KA>
__global__ __launch_bounds__(256, 2) void linear_fwd_pair_kernel(LinearParams a, LinearParams b, int nb_b) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[linear_lds_bytes<(KA > KB ? KA : KB)>()];
  if ((int)blockIdx.x < nb_b) linear_fwd_body<T, KB>(b, blockIdx.x, lds);
  else linear_fwd_body<T, KA>(a, (int64_t)blockIdx.x - nb_b, lds);
}

// ---- resident-W form for large row counts ----------------------------------------------------------------------
// The chunked kernel above keeps four 128-row blocks per CU, each of which lives ~25 us for ~3 us of matrix work: two
// barriers per 64-column chunk, W re-committed to LDS per chunk and block, the X fragments loaded with nothing to
// overlap.  Bytes in flight per CU / block lifetime is what bounds it (4.3 TB/s of stores with the loads taken out,
// 1.97 TB/s of loads with the stores taken out: `EXP_NOLOAD` / `EXP_NOSTORE` builds, round 3).  For n >= ~10^5 rows
// and K * M small enough, ONE persistent workgroup per CU holds the whole W in LDS (384 x 128 bf16 = 102 KB with the
// conflict-free row stride) and its 12 waves walk 32-row tiles on their own: no barrier after the W load, the next
// tile's X fragments requested before the current tile's MFMAs, the epilogue tile wave-private.  NCH (chunks of 64
// output columns) is a template parameter so that the chunk loop is straight-line code: the wait for the prefetched
// X fragments is then vmcnt(4 * NCH) -- the tile's output stores stay in flight (gfx9 counts stores in vmcnt).
constexpr int kResWaves = 12;
constexpr int kResMaxOut = 384;

template <typename T, int K, int NCH>
__global__ __launch_bounds__(kResWaves * 64, 1) void linear_res_kernel(LinearParams p, int64_t n_tiles) {
  constexpr int NK = K / 16;
  constexpr int WSTRIDE = K * 2 + 16;
  constexpr int ESTRIDE = kChunk * 2 + 16;
  constexpr int M = NCH * kChunk;
  __shared__ __attribute__((aligned(16))) unsigned char lds[M * WSTRIDE + kResWaves * 32 * ESTRIDE];
  __shared__ __attribute__((aligned(16))) float lds_bias[M];
  unsigned char* lds_w = lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  unsigned char* et = lds + M * WSTRIDE + wave * 32 * ESTRIDE;
  const T* __restrict__ x = static_cast<const T*>(p.x);
  const T* __restrict__ w = static_cast<const T*>(p.w);
  T* __restrict__ y = static_cast<T*>(p.y);

  for (int piece = tid; piece < M * K / 8; piece += kResWaves * 64) {
    const int wrow = piece / (K / 8), wcol = piece % (K / 8);
    *reinterpret_cast<u32x4*>(lds_w + wrow * WSTRIDE + wcol * 16) = *reinterpret_cast<const u32x4*>(w + (int64_t)wrow * K + wcol * 8);
  }
  for (int i = tid; i < M; i += kResWaves * 64) lds_bias[i] = p.bias ? p.bias[i] : 0.f;
  __syncthreads();

  const int64_t stride = (int64_t)gridDim.x * kResWaves;
  int64_t tile = (int64_t)blockIdx.x * kResWaves + wave;          // at any time the grid covers one contiguous run of tiles
  const int64_t n_full = p.n_rows / 32;                           // tiles without a missing row

  auto x_load = [&](u32x4 (&dst)[NK], int64_t t) {
    int64_t row = t * 32 + r;
    if (row >= p.n_rows) row = p.n_rows - 1;                      // clamp: loaded, never stored
    const T* xr = x + row * p.ldx + 8 * h;
#pragma unroll
    for (int s = 0; s < NK; ++s) dst[s] = *reinterpret_cast<const u32x4*>(xr + 16 * s);
  };

  u32x4 xb[NK], xn[NK];
  if (tile < n_tiles) x_load(xn, tile);

  auto do_tile = [&](auto full_c, const int64_t t) {
    constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
    for (int s = 0; s < NK; ++s) xb[s] = xn[s];
    if (t + stride < n_tiles) x_load(xn, t + stride);             // under this tile's MFMAs
    const int64_t row0 = t * 32;
    // NCH == 2 (M = 128): fully unrolled the two chunks' MFMA chains and epilogues are interleaved by the scheduler and the
    // tile loop spills 136 bytes per lane (7 reloads inside it); kept as a loop the kernel needs no scratch
#pragma unroll NCH == 2 ? 1 : NCH
    for (int c = 0; c < NCH; ++c) {
      const int c0 = c * kChunk;
      f32x16 acc[2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
      }
#pragma unroll
      for (int s = 0; s < NK; ++s) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const u32x4 a = *reinterpret_cast<const u32x4*>(lds_w + (c0 + ct * 32 + r) * WSTRIDE + (16 * s + 8 * h) * 2);
          acc[ct] = Mfma<T>::run(a, xb[s], acc[ct]);
        }
      }
      // epilogue through the wave's own LDS tile (LDS operations of one wave execute in order: no barrier)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = ct * 32 + 8 * g + 4 * h;
          const f32x4 bv = *reinterpret_cast<const f32x4*>(lds_bias + c0 + col);
          uint2 pk;
          pk.x = Vec8<T>::pack(acc[ct][4 * g + 0] + bv.x, acc[ct][4 * g + 1] + bv.y);
          pk.y = Vec8<T>::pack(acc[ct][4 * g + 2] + bv.z, acc[ct][4 * g + 3] + bv.w);
          *reinterpret_cast<uint2*>(et + r * ESTRIDE + col * 2) = pk;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int er = 8 * i + (lane >> 3), piece = lane & 7;
        const u32x4 v = *reinterpret_cast<const u32x4*>(et + er * ESTRIDE + piece * 16);
        const int64_t row = row0 + er;
        if (FULL || row < p.n_rows) *reinterpret_cast<u32x4*>(y + row * p.ldy + c0 + piece * 8) = v;
      }
    }
  };
  // full tiles: unconditional stores (events the wait-count analysis can count on); the one partial tile afterwards
#pragma unroll 1
  for (; tile < n_full; tile += stride) do_tile(std::true_type{}, tile);
  if (tile < n_tiles) do_tile(std::false_type{}, tile);
}

// ---- host: the entry points fill a FwdRequest, plan_fwd checks and routes, one executor per unit launches -------
#define K_IS(KK) || k == KK
#define K_TEXT(KK) " " #KK
#define RES_IS(KK, NN) || (k == KK && m == NN * kChunk)
bool chunked_k(int k) { return false SEGGER_FWD_K_LIST(K_IS); }
bool f32_epilogue_k(int k) { return false SEGGER_FWD_F32_EPILOGUE_K_LIST(K_IS); }
bool resident_shape(int k, int m) { return false SEGGER_FWD_RES_LIST(RES_IS); }
bool out_width_ok(int m) { return m > 0 && m % kChunk == 0; }
// (no list where one kernel serves: the planes' chunked <128> / <384>, the row bias' two K, the SiLU' K, the K-slice, 384 + 128)
bool split_shape(int k, int m) { return (k == 128 && out_width_ok(m)) || (k == 384 && m == 128); }

LinearParams params_16(const FwdRequest& q) {
  LinearParams p{};
  p.x = q.x;  p.ldx = q.ldx;  p.w = q.w;  p.bias = q.bias;
  p.y = q.y;  p.ldy = q.ldy;  p.n_rows = q.n_rows;  p.m_out = q.m_out;
  if (q.has_rowbias) { p.rowbias = q.rowbias;  p.rowidx = q.rowidx;  p.ld_rb = q.ld_rb; }
  if (q.gate_form == FwdGate::kSilu16) { p.gate = q.gate;  p.ld_gate = q.ld_gate; }
  return p;
}

template <typename T>
int launch_fwd_16(const FwdRequest& q, const FwdPlan& plan, hipStream_t stream) {
  const LinearParams p = params_16(q);
  const dim3 grid((unsigned)plan.grid), block(256);
#define RES(KK, NN) else if (q.k_in == KK && q.m_out == NN * kChunk) hipLaunchKernelGGL( \
    (linear_res_kernel<T, KK, NN>), grid, dim3(kResWaves * 64), 0, stream, p, ceil_div(q.n_rows, 32));
#define CHUNKED(KK) else if (q.k_in == KK) hipLaunchKernelGGL((linear_fwd_kernel<T, KK>), grid, block, 0, stream, p);
  if (plan.route == FwdRoute::kRes16) { if (false) {} SEGGER_FWD_RES_LIST(RES) }
  else if (plan.route == FwdRoute::kSiluGrad16)
    hipLaunchKernelGGL((linear_fwd_kernel<T, 64, false, true>), grid, block, 0, stream, p);
  else if (plan.route == FwdRoute::kRowBias16 && q.k_in == 64)
    hipLaunchKernelGGL((linear_fwd_kernel<T, 64, true>), grid, block, 0, stream, p);
  else if (plan.route == FwdRoute::kRowBias16) hipLaunchKernelGGL((linear_fwd_kernel<T, 128, true>), grid, block, 0, stream, p);
  else { if (false) {} SEGGER_FWD_K_LIST(CHUNKED) }
#undef RES
#undef CHUNKED
  SEGGER_LAUNCH_CHECK("linear_fwd_kernel / linear_res_kernel");
  return SEGGER_OK;
}

// both sides' 128-row blocks in one grid, b's first (two plain chunked projections of one K, or of the two-width pair)
template <typename T>
int launch_fwd_pair_16(const FwdRequest& qa, const FwdRequest& qb, int64_t nb_a, int64_t nb_b, hipStream_t stream) {
  const LinearParams a = params_16(qa), b = params_16(qb);
  const dim3 grid((unsigned)(nb_a + nb_b)), block(256);
#define SAME(KK) else if (qa.k_in == KK) hipLaunchKernelGGL((linear_fwd_pair_kernel<T, KK>), grid, block, 0, stream, a, b, (int)nb_b);
  if (qa.k_in != qb.k_in) hipLaunchKernelGGL((linear_fwd_pair_kernel<T, 384, 128>), grid, block, 0, stream, a, b, (int)nb_b);
  SEGGER_FWD_K_LIST(SAME)
#undef SAME
  SEGGER_LAUNCH_CHECK("linear_fwd_pair_kernel");
  return SEGGER_OK;
}

int launch_fwd(const FwdRequest& q, const FwdPlan& plan, hipStream_t stream) {
  switch (plan.route) {
    case FwdRoute::kNone: return SEGGER_OK;
    case FwdRoute::kExactF32: case FwdRoute::kKSliceF32: return launch_fwd_f32(q, plan, stream);
    case FwdRoute::kSplit: return launch_fwd_f32_split(q, plan, stream);
    default: return q.dtype == SEGGER_BF16 ? launch_fwd_16<bf16_t>(q, plan, stream) : launch_fwd_16<f16_t>(q, plan, stream);
  }
}

int run_fwd(const FwdRequest& q, segger_stream_t stream) {
  FwdPlan plan;
  const int rc = plan_fwd(q, &plan);
  return rc != SEGGER_OK ? rc : launch_fwd(q, plan, (hipStream_t)stream);
}

// The pair: both sides are planned before anything runs.  One joint launch where both are plain chunked 16-bit projections
// of one K (or 384 beside 128); otherwise each side goes its own planned way, a side without rows nowhere.
int run_fwd_pair(const FwdRequest& a, const FwdRequest& b, hipStream_t stream) {
  FwdPlan pa, pb;
  int rc = plan_fwd(a, &pa);
  if (rc == SEGGER_OK) rc = plan_fwd(b, &pb);
  if (rc != SEGGER_OK) return rc;
  const int64_t nb_a = ceil_div(a.n_rows, kRowsPerBlock), nb_b = ceil_div(b.n_rows, kRowsPerBlock);
  const bool b_plain16 = pb.route == FwdRoute::kChunk16 || pb.route == FwdRoute::kRes16;   // (beside a small a, b is not asked)
  const bool k_joint = a.k_in == b.k_in || (a.k_in == 384 && b.k_in == 128);
  if (pa.route == FwdRoute::kChunk16 && b_plain16 && k_joint && nb_a + nb_b <= 0x7fffffffLL)
    return a.dtype == SEGGER_BF16 ? launch_fwd_pair_16<bf16_t>(a, b, nb_a, nb_b, stream)
                                  : launch_fwd_pair_16<f16_t>(a, b, nb_a, nb_b, stream);
  rc = launch_fwd(a, pa, stream);
  return rc != SEGGER_OK ? rc : launch_fwd(b, pb, stream);
}

}  // namespace

// Every host check of a forward projection, once and in this order: sizes; act_kind / gate_kind; the shape (in the called
// entry's name); NULL pointers; 16-byte alignment; leading dimensions; the row bias table; then the route, its grid and the
// row count.  What a call without rows still answers for is the request's to say (shape_before_empty, pair_side: common.h).
// The element size (esize, post_common.h) is all that differs between the storage widths.
int plan_fwd(const FwdRequest& q, FwdPlan* plan) {
  const int k = q.k_in, m = q.m_out;
  const bool f32 = q.dtype == SEGGER_F32, sixteen = q.dtype == SEGGER_BF16 || q.dtype == SEGGER_F16, none = q.n_rows == 0;
  const bool gate_f32 = q.gate_form == FwdGate::kF32, silu16 = q.gate_form == FwdGate::kSilu16;
  const bool f32_only = q.w_planes || gate_f32 || q.has_act;
  // (the fp32-only forms leave k_in and m_out, a 16-bit pair side k_in, to the shape: unsupported, not a bad argument)
  SEGGER_REQUIRE(q.n_rows >= 0 && (f32_only || (m > 0 && (k > 0 || q.pair_side))),
                 "%s: bad sizes (negative n_rows, k_in or m_out not positive)", q.who);
  SEGGER_REQUIRE(!q.has_act || q.act_kind == 1 || q.act_kind == 2, "%s: act_kind 1 (GELU) or 2 (SiLU)", q.who);
  SEGGER_REQUIRE(!gate_f32 || q.gate_kind == 1 || q.gate_kind == 2, "%s: gate_kind 1 (GELU) or 2 (SiLU)", q.who);
  *plan = FwdPlan{FwdRoute::kNone, ceil_div(q.n_rows, kRowsPerBlock)};      // (the grid of every route but the persistent one)
  if (none && !q.shape_before_empty) return SEGGER_OK;
  SEGGER_REQUIRE(!silu16 || (k == 64 && out_width_ok(m) && sixteen), "%s: k_in 64, m_out %% 64 == 0, bf16 / f16", q.who);
  const bool f32_epilogue = gate_f32 || q.has_act || (f32 && q.has_rowbias);
  const bool k_ok = f32_epilogue ? f32_epilogue_k(k) : q.has_rowbias ? (k == 64 || k == 128) : chunked_k(k);
  if (!(q.w_planes ? split_shape(k, m) : (f32 || sixteen) && out_width_ok(m) && k_ok)) {
    set_error("%s: k_in=%d m_out=%d dtype=%d not supported (m_out %% 64 == 0; k_in" SEGGER_FWD_K_LIST(K_TEXT) ", with a row bias 64 128,"
              " with an fp32 epilogue" SEGGER_FWD_F32_EPILOGUE_K_LIST(K_TEXT) "; planes 128 -> any, 384 -> 128)", q.who, k, m, q.dtype);
    return SEGGER_EUNSUPPORTED;
  }
  if (none && !q.pair_side) return SEGGER_OK;
  // (an operand that the form does not have is NULL in the request: aligned, and its leading dimension is not asked)
  SEGGER_REQUIRE(none || (q.x && q.w && q.y && (q.gate_form == FwdGate::kNone || q.gate) && (!q.has_act || q.y_act)),
                 "%s: NULL pointer", q.who);
  SEGGER_REQUIRE(!q.has_rowbias || (q.rowbias && q.rowidx), "%s: the rowbias table and rowidx go together", q.who);
  SEGGER_REQUIRE(is_aligned(q.x, 16) && is_aligned(q.w, 16) && is_aligned(q.y, 16) && is_aligned(q.gate, 16) &&
                     is_aligned(q.y_act, 16) && (!f32 || is_aligned(q.bias, 16)),
                 "%s: pointers (at fp32 the bias too) must be 16-byte aligned", q.who);
  const int64_t es = (int64_t)esize(q.dtype);
  const auto ld_ok = [&](int64_t ld, int64_t width, int bytes) { return ld >= width && (ld * es) % bytes == 0; };
  SEGGER_REQUIRE(ld_ok(q.ldx, k, 16) && ld_ok(q.ldy, m, 16) && (!q.gate || ld_ok(q.ld_gate, m, silu16 ? 8 : 16)) &&
                     (!q.y_act || ld_ok(q.ld_yact, m, 16)),
                 "%s: bad leading dimension (shorter than a row, or rows not 16-byte aligned)", q.who);
  SEGGER_REQUIRE(!q.has_rowbias || (is_aligned(q.rowbias, 16) && ld_ok(q.ld_rb, m, 16)),
                 "%s: the rowbias table needs 16-byte aligned rows of at least m_out elements", q.who);
  if (none) return SEGGER_OK;
  // the persistent form is worth it only when every wave of its grid gets a few 32-row tiles
  const bool plain16 = sixteen && !silu16 && !q.has_rowbias;
  const int n_cu = plain16 && resident_shape(k, m) ? device_cu_count() : 0;           // per device (common.h)
  const bool res = n_cu > 0 && ceil_div(q.n_rows, 32) >= (int64_t)n_cu * kResWaves * 2;
  if (res) plan->grid = n_cu;
  plan->route = q.w_planes ? FwdRoute::kSplit
              : f32 ? (k == 384 && (m == 128 || m == 256) ? FwdRoute::kKSliceF32 : FwdRoute::kExactF32)
              : silu16 ? FwdRoute::kSiluGrad16 : q.has_rowbias ? FwdRoute::kRowBias16 : res ? FwdRoute::kRes16 : FwdRoute::kChunk16;
  if (plan->grid > 0x7fffffffLL) {
    set_error("%s: too many rows", q.who);
    return q.w_planes ? SEGGER_EINVAL : SEGGER_EUNSUPPORTED;                 // (as either family has always answered)
  }
  return SEGGER_OK;
}

}  // namespace segger

using namespace segger;

extern "C" int segger_linear_supported(int32_t k_in, int32_t m_out, int32_t dtype) {
  return chunked_k(k_in) && out_width_ok(m_out) && (dtype == SEGGER_BF16 || dtype == SEGGER_F16 || dtype == SEGGER_F32);
}

extern "C" int segger_linear_fwd_f32_split_supported(int32_t k_in, int32_t m_out) { return split_shape(k_in, m_out); }

// the fields every form has; an entry point adds its own by name
static FwdRequest request(const char* who, int32_t dtype, int64_t n_rows, int32_t k_in, int32_t m_out, const void* x, int64_t ldx,
                          const void* w, const float* bias, void* y, int64_t ldy) {
  FwdRequest q;
  q.who = who;  q.dtype = dtype;  q.n_rows = n_rows;  q.k_in = k_in;  q.m_out = m_out;
  q.x = x;  q.ldx = ldx;  q.w = w;  q.bias = bias;  q.y = y;  q.ldy = ldy;
  return q;
}

extern "C" int segger_linear_fwd_pair(const segger_linear_args* a, const segger_linear_args* b, int32_t k_in, int32_t dtype,
                                      segger_stream_t stream) {
  return segger_linear_fwd_pair_k(a, k_in, b, k_in, dtype, stream);
}

extern "C" int segger_linear_fwd_pair_k(const segger_linear_args* a, int32_t k_a, const segger_linear_args* b, int32_t k_b,
                                        int32_t dtype, segger_stream_t stream) {
  SEGGER_REQUIRE(a && b, "segger_linear_fwd_pair: NULL args");
  const char* who = "segger_linear_fwd_pair";
  FwdRequest qa = request(who, dtype, a->n_rows, k_a, a->m_out, a->x, a->ldx, a->w, a->bias, a->y, a->ldy);
  FwdRequest qb = request(who, dtype, b->n_rows, k_b, b->m_out, b->x, b->ldx, b->w, b->bias, b->y, b->ldy);
  qa.shape_before_empty = qa.pair_side = qb.shape_before_empty = qb.pair_side = dtype != SEGGER_F32;   // (fp32: as two plain calls)
  return run_fwd_pair(qa, qb, (hipStream_t)stream);
}

extern "C" int segger_linear_fwd(const void* x, int64_t ldx, const void* w, const float* bias, void* y, int64_t ldy,
                                 int64_t n_rows, int32_t k_in, int32_t m_out, int32_t dtype, segger_stream_t stream) {
  return run_fwd(request("segger_linear_fwd", dtype, n_rows, k_in, m_out, x, ldx, w, bias, y, ldy), stream);
}

extern "C" int segger_linear_fwd_rowbias(const void* x, int64_t ldx, const void* w, const float* bias, const void* rowbias,
                                         int64_t ld_rb, const int32_t* rowidx, void* y, int64_t ldy, int64_t n_rows,
                                         int32_t k_in, int32_t m_out, int32_t dtype, segger_stream_t stream) {
  FwdRequest q = request("segger_linear_fwd_rowbias", dtype, n_rows, k_in, m_out, x, ldx, w, bias, y, ldy);
  q.has_rowbias = rowbias || rowidx;  q.rowbias = rowbias;  q.rowidx = rowidx;  q.ld_rb = ld_rb;
  return run_fwd(q, stream);
}

extern "C" int segger_linear_fwd_silu_grad(const void* x, int64_t ldx, const void* w, const void* gate, int64_t ld_gate,
                                           void* y, int64_t ldy, int64_t n_rows, int32_t k_in, int32_t m_out,
                                           int32_t dtype, segger_stream_t stream) {
  FwdRequest q = request("segger_linear_fwd_silu_grad", dtype, n_rows, k_in, m_out, x, ldx, w, nullptr, y, ldy);
  q.gate_form = FwdGate::kSilu16;  q.gate = gate;  q.ld_gate = ld_gate;
  return run_fwd(q, stream);
}

extern "C" int segger_linear_fwd_f32_split(const float* x, int64_t ldx, const void* w3, const float* bias, float* y, int64_t ldy,
                                           int64_t n_rows, int32_t k_in, int32_t m_out, segger_stream_t stream) {
  FwdRequest q = request("segger_linear_fwd_f32_split", SEGGER_F32, n_rows, k_in, m_out, x, ldx, w3, bias, y, ldy);
  q.w_planes = q.shape_before_empty = true;
  return run_fwd(q, stream);
}

extern "C" int segger_linear_fwd_f32_split_rowbias(const float* x, int64_t ldx, const void* w3, const float* rowbias, int64_t ld_rb,
                                                   const int32_t* rowidx, float* y, int64_t ldy, int64_t n_rows, int32_t k_in,
                                                   int32_t m_out, segger_stream_t stream) {
  FwdRequest q = request("segger_linear_fwd_f32_split_rowbias", SEGGER_F32, n_rows, k_in, m_out, x, ldx, w3, nullptr, y, ldy);
  q.w_planes = q.shape_before_empty = q.has_rowbias = true;  q.rowbias = rowbias;  q.rowidx = rowidx;  q.ld_rb = ld_rb;
  return run_fwd(q, stream);
}

extern "C" int segger_linear_fwd_f32_act(const float* x, int64_t ldx, const float* w, const float* bias, float* y, int64_t ldy,
                                         float* y_act, int64_t ld_yact, int32_t act_kind, int64_t n_rows, int32_t k_in,
                                         int32_t m_out, segger_stream_t stream) {
  FwdRequest q = request("segger_linear_fwd_f32_act", SEGGER_F32, n_rows, k_in, m_out, x, ldx, w, bias, y, ldy);
  q.has_act = true;  q.y_act = y_act;  q.ld_yact = ld_yact;  q.act_kind = act_kind;
  return run_fwd(q, stream);
}

extern "C" int segger_linear_fwd_f32_gate(const float* x, int64_t ldx, const void* w, int32_t w_is_planes, const float* gate,
                                          int64_t ld_gate, int32_t gate_kind, float* y, int64_t ldy, int64_t n_rows, int32_t k_in,
                                          int32_t m_out, segger_stream_t stream) {
  FwdRequest q = request("segger_linear_fwd_f32_gate", SEGGER_F32, n_rows, k_in, m_out, x, ldx, w, nullptr, y, ldy);
  q.w_planes = w_is_planes != 0;  q.gate_form = FwdGate::kF32;  q.gate = gate;  q.ld_gate = ld_gate;  q.gate_kind = gate_kind;
  return run_fwd(q, stream);
}
