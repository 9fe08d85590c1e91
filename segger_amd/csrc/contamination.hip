// segger_neighbor_frequencies / segger_contamination_posterior: the two kernels behind segger_amd.validation
// (include/segger_amd.h has the contract; the reference is src/segger/validation/contamination.py).
//
// Frequencies: one wave per cell.  Lane j holds neighbour j of the [n, k] table (k <= 64) and its label, or -1 when the
// neighbour does not count (padding, farther than max_distance, unlabelled); lane l then owns the types l, l + 64,
// l + 128, l + 192 and counts the lanes that hold each of them by reading the k labels back one lane at a time.  Every
// element of counts / freq is written once, by its owner: no atomics.
//
// Posterior: one wave per CSR row.  The row's T frequencies are staged in a wave-private LDS strip with the host type's
// slot zeroed; lanes take the stored entries 64 at a time and each sums freq[r, t] * L[t, g] over ascending t in float64
// from the gene-major table Lt [G_ref, ld] -- 16 bytes (four types) per read.  The table is copied into LDS once per
// workgroup when it fits SEGGER_CONTAM_LDS_BYTES next to the strips (the grid is then as many workgroups per CU as the
// CU's LDS holds copies, up to its 32 wave slots), and is read through L2 otherwise.  In LDS a gene's
// row is ld_s floats with ld_s / 4 odd: the 16-lane groups of a ds_read_b128 hit slot (g * ld_s / 4 + t / 4) mod 16, which
// an odd multiplier spreads over all 16 slots for lanes with different g (an even one folds them onto 8, 4, 2 or 1).
// Nothing of size nnz x T is built; the two integer sums of a row are one wave reduction; the same bits from call to call.
#include <math.h>

#include "common.h"
#include "post_common.h"

namespace segger {
namespace {

constexpr int kContamThreads = 256;
constexpr int kContamWaves = kContamThreads / kWave;
constexpr size_t kCuLdsBytes = 160 * 1024;                       // LDS of one CU of gfx950
constexpr int kMaxGroupsPerCu = 2048 / kContamThreads;           // 32 wave slots per CU
constexpr int kTypeChunks = SEGGER_CONTAM_MAX_TYPES / kWave;     // types per lane in the frequency kernel

static_assert(SEGGER_CONTAM_MAX_TYPES % kWave == 0, "a lane owns whole 64-type chunks");
static_assert(SEGGER_CONTAM_MAX_K <= kWave, "one lane per neighbour");

__global__ __launch_bounds__(kContamThreads) void neighbor_frequencies_kernel(
    const int32_t* __restrict__ nbr, const float* __restrict__ dist, const int32_t* __restrict__ labels, int64_t n, int k, int T,
    double max_distance, int32_t* __restrict__ counts, float* __restrict__ freq) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t n_waves = (int64_t)gridDim.x * kContamWaves;
  for (int64_t r = (int64_t)blockIdx.x * kContamWaves + (threadIdx.x >> 6); r < n; r += n_waves) {      // wave-uniform
    int lab = -1;
    if (lane < k) {
      const int32_t j = nbr[r * k + lane];
      if ((uint32_t)j < (uint32_t)n && (double)dist[r * k + lane] <= max_distance) {    // padding (id n) is never an index
        const int32_t l = labels[j];
        if ((uint32_t)l < (uint32_t)T) lab = l;
      }
    }
    const int sum = __popcll(__ballot(lab >= 0));
    int cnt[kTypeChunks];
#pragma unroll
    for (int c = 0; c < kTypeChunks; ++c) cnt[c] = 0;
    for (int j = 0; j < k; ++j) {
      const int lj = __shfl(lab, j, kWave);
#pragma unroll
      for (int c = 0; c < kTypeChunks; ++c) cnt[c] += lj == lane + c * kWave;
    }
    const double inv = sum > 0 ? 1.0 / (double)sum : 0.0;
#pragma unroll
    for (int c = 0; c < kTypeChunks; ++c) {
      const int t = lane + c * kWave;
      if (t < T) {
        counts[r * T + t] = cnt[c];
        freq[r * T + t] = (float)((double)cnt[c] * inv);
      }
    }
  }
}

struct PosteriorArgs {
  const int64_t* indptr; const int32_t* indices; const int32_t* counts;
  int64_t n_rows, n_cols, nnz;
  const int32_t* gene_map; const int32_t* host_type; const float* freq; const float* Lt; int64_t ld_L; const double* back;
  int T, G_ref, ld_s;
  double alpha_self, alpha_neighbor, alpha_background, eps, cutoff;
  float* q_self; float* q_neighbor; float* q_background; int32_t* contamination;
  int64_t* contaminated; int64_t* total; double* percent;
};

// kLds: the table sits in LDS (row stride a.ld_s) in front of the frequency strips; otherwise rows of a.Lt are read
template <bool kLds>
__global__ __launch_bounds__(kContamThreads) void contamination_posterior_kernel(const PosteriorArgs a) {
  extern __shared__ __align__(16) float smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int T = a.T;
  const int Tp = (T + 3) & ~3;
  const int64_t table_floats = kLds ? (int64_t)a.G_ref * a.ld_s : 0;
  if (kLds) {
    const int64_t n_elem = (int64_t)a.G_ref * T;
    for (int64_t i = threadIdx.x; i < n_elem; i += kContamThreads) {
      const int64_t g = i / T;
      const int t = (int)(i - g * T);
      smem[g * a.ld_s + t] = a.Lt[g * a.ld_L + t];
    }
    __syncthreads();
  }
  float* fr = smem + table_floats + wave * Tp;
  const int full = T >> 2;
  const int64_t n_waves = (int64_t)gridDim.x * kContamWaves;
  for (int64_t r = (int64_t)blockIdx.x * kContamWaves + wave; r < a.n_rows; r += n_waves) {              // wave-uniform
    int type = a.host_type[r];
    if ((uint32_t)type >= (uint32_t)T) type = -1;        // a label outside [0, T) is no label: never an index
    __builtin_amdgcn_wave_barrier();                     // the strip is wave-private: one wave's LDS ops stay in order
    for (int t = lane; t < Tp; t += kWave) fr[t] = (t < T && t != type) ? a.freq[r * T + t] : 0.0f;
    __builtin_amdgcn_wave_barrier();
    int64_t beg = a.indptr[r], end = a.indptr[r + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > a.nnz ? a.nnz : end;                     // never past the arrays, whatever indptr holds
    int64_t flagged = 0, total = 0;
    for (int64_t e = beg + lane; e < end; e += kWave) {
      const int32_t col = a.indices[e];
      const int32_t v = a.counts[e];
      int32_t g = (uint32_t)col < (uint32_t)a.n_cols ? a.gene_map[col] : -1;
      if ((uint32_t)g >= (uint32_t)a.G_ref) g = -1;
      total += v;
      double qs = 0.0, qn = 0.0, qb = 0.0;
      int32_t flag = 0;
      if (g >= 0) {
        const float* row = kLds ? smem + (int64_t)g * a.ld_s : a.Lt + (int64_t)g * a.ld_L;
        const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
        const f32x4* fr4 = reinterpret_cast<const f32x4*>(fr);
        double acc = 0.0;
        for (int t4 = 0; t4 < full; ++t4) {
          const f32x4 l = row4[t4];
          const f32x4 f = fr4[t4];
          acc = fma((double)f.x, (double)l.x, acc);
          acc = fma((double)f.y, (double)l.y, acc);
          acc = fma((double)f.z, (double)l.z, acc);
          acc = fma((double)f.w, (double)l.w, acc);
        }
        for (int t = full * 4; t < T; ++t) acc = fma((double)fr[t], (double)row[t], acc);
        const double p_self = type >= 0 ? (double)row[type] : a.eps;
        qs = a.alpha_self * p_self;
        qn = a.alpha_neighbor * (acc + a.eps);
        qb = a.alpha_background * (a.back[g] + a.eps);
        const double denom = qs + qn + qb;
        qs /= denom;
        qn /= denom;
        qb /= denom;
        if (qs < a.cutoff) {
          flag = v;
          flagged += v;
        }
      }
      a.q_self[e] = (float)qs;
      a.q_neighbor[e] = (float)qn;
      a.q_background[e] = (float)qb;
      a.contamination[e] = flag;
    }
    flagged = wave_sum_i64(flagged);
    total = wave_sum_i64(total);
    if (lane == 0) {
      a.contaminated[r] = flagged;
      a.total[r] = total;
      a.percent[r] = 100.0 * (double)flagged / (double)(total > 1 ? total : 1);
    }
  }
}

// LDS row stride of the table in floats (ld_s / 4 odd), or 0 when table + strips pass the budget
int posterior_lds_stride(int T, int G_ref) {
  const int Tp = (T + 3) & ~3;
  const int ld_s = (Tp / 4) % 2 ? Tp : Tp + 4;
  const int64_t bytes = ((int64_t)G_ref * ld_s + (int64_t)kContamWaves * Tp) * (int64_t)sizeof(float);
  return bytes <= SEGGER_CONTAM_LDS_BYTES ? ld_s : 0;
}

int64_t contam_grid(int64_t n_rows, int groups_per_cu) {
  int64_t blocks = ceil_div(n_rows, kContamWaves);
  const int cus = device_cu_count();
  const int64_t cap = (int64_t)(cus > 0 ? cus : 256) * groups_per_cu;
  return blocks < cap ? blocks : cap;
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" int segger_neighbor_frequencies(const int32_t* nbr, const float* dist, const int32_t* labels, int64_t n, int32_t k,
                                           int32_t n_types, double max_distance, int32_t* counts, float* freq,
                                           segger_stream_t stream_) {
  const char* who = "segger_neighbor_frequencies";
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n >= 0, "%s: negative n", who);
  SEGGER_REQUIRE(n < 0x7fffffffLL, "%s: 2^31 - 1 points or more", who);
  SEGGER_REQUIRE(k >= 1 && k <= SEGGER_CONTAM_MAX_K, "%s: k = %d outside 1 .. %d", who, (int)k, SEGGER_CONTAM_MAX_K);
  SEGGER_REQUIRE(n_types >= 1 && n_types <= SEGGER_CONTAM_MAX_TYPES, "%s: n_types = %d outside 1 .. %d", who, (int)n_types,
                 SEGGER_CONTAM_MAX_TYPES);
  SEGGER_REQUIRE(max_distance >= 0.0, "%s: max_distance must be >= 0 (+inf for none)", who);             // NaN fails too
  if (n == 0) return SEGGER_OK;
  SEGGER_REQUIRE(nbr && dist && labels && counts && freq, "%s: NULL pointer", who);
  SEGGER_REQUIRE(is_aligned(nbr, 4) && is_aligned(dist, 4) && is_aligned(labels, 4) && is_aligned(counts, 4) &&
                     is_aligned(freq, 4), "%s: every array must be 4-byte aligned", who);
  hipLaunchKernelGGL(neighbor_frequencies_kernel, dim3((unsigned)contam_grid(n, 16)), dim3(kContamThreads), 0, stream, nbr, dist,
                     labels, n, (int)k, (int)n_types, max_distance, counts, freq);
  SEGGER_LAUNCH_CHECK("neighbor_frequencies_kernel");
  return SEGGER_OK;
}

extern "C" int segger_contamination_posterior(
    const int64_t* indptr, const int32_t* indices, const int32_t* counts, int64_t n_rows, int64_t n_cols, int64_t nnz,
    const int32_t* gene_map, const int32_t* host_type, const float* freq, const float* Lt, int64_t ld_L, const double* back,
    int32_t n_types, int32_t n_ref_genes, double alpha_self, double alpha_neighbor, double alpha_background, double eps,
    double contam_cutoff, float* q_self, float* q_neighbor, float* q_background, int32_t* contamination, int64_t* contaminated,
    int64_t* total, double* percent, segger_stream_t stream_) {
  const char* who = "segger_contamination_posterior";
  hipStream_t stream = (hipStream_t)stream_;
  SEGGER_REQUIRE(n_rows >= 0 && n_cols >= 0, "%s: negative n_rows or n_cols", who);
  SEGGER_REQUIRE(n_rows < 0x7fffffffLL && n_cols < 0x7fffffffLL, "%s: 2^31 - 1 rows or columns or more", who);
  SEGGER_REQUIRE(nnz >= 0, "%s: negative nnz", who);
  SEGGER_REQUIRE(n_types >= 1 && n_types <= SEGGER_CONTAM_MAX_TYPES, "%s: n_types = %d outside 1 .. %d", who, (int)n_types,
                 SEGGER_CONTAM_MAX_TYPES);
  SEGGER_REQUIRE(n_ref_genes >= 1 && n_ref_genes <= SEGGER_CONTAM_MAX_REF_GENES, "%s: n_ref_genes = %d outside 1 .. %d", who,
                 (int)n_ref_genes, SEGGER_CONTAM_MAX_REF_GENES);
  SEGGER_REQUIRE(ld_L >= n_types && ld_L % 4 == 0 && ld_L <= 0x7fffffffLL, "%s: ld_L must be a multiple of 4 and >= n_types", who);
  SEGGER_REQUIRE(isfinite(alpha_self) && isfinite(alpha_neighbor) && isfinite(alpha_background),
                 "%s: alpha_self, alpha_neighbor and alpha_background must be finite", who);
  SEGGER_REQUIRE(isfinite(eps), "%s: eps must be finite", who);
  SEGGER_REQUIRE(!isnan(contam_cutoff), "%s: contam_cutoff is NaN", who);
  if (n_rows == 0 || nnz == 0) return SEGGER_OK;         // nothing stored: nothing is written (the caller zero-fills)
  SEGGER_REQUIRE(indptr && indices && counts && gene_map && host_type && freq && Lt && back, "%s: NULL pointer", who);
  SEGGER_REQUIRE(n_cols >= 1, "%s: stored entries but n_cols = 0", who);
  SEGGER_REQUIRE(q_self && q_neighbor && q_background && contamination && contaminated && total && percent, "%s: NULL pointer",
                 who);
  SEGGER_REQUIRE(is_aligned(indptr, 8) && is_aligned(back, 8) && is_aligned(contaminated, 8) &&
                     is_aligned(total, 8) && is_aligned(percent, 8),
                 "%s: indptr, back, contaminated, total and percent must be 8-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(indices, 4) && is_aligned(counts, 4) && is_aligned(gene_map, 4) &&
                     is_aligned(host_type, 4) && is_aligned(freq, 4) && is_aligned(q_self, 4) &&
                     is_aligned(q_neighbor, 4) && is_aligned(q_background, 4) && is_aligned(contamination, 4),
                 "%s: every 32-bit array must be 4-byte aligned", who);
  SEGGER_REQUIRE(is_aligned(Lt, 16), "%s: Lt must be 16-byte aligned", who);
  PosteriorArgs a;
  a.indptr = indptr; a.indices = indices; a.counts = counts;
  a.n_rows = n_rows; a.n_cols = n_cols; a.nnz = nnz;
  a.gene_map = gene_map; a.host_type = host_type; a.freq = freq; a.Lt = Lt; a.ld_L = ld_L; a.back = back;
  a.T = (int)n_types; a.G_ref = (int)n_ref_genes; a.ld_s = posterior_lds_stride(a.T, a.G_ref);
  a.alpha_self = alpha_self; a.alpha_neighbor = alpha_neighbor; a.alpha_background = alpha_background; a.eps = eps;
  a.cutoff = contam_cutoff;
  a.q_self = q_self; a.q_neighbor = q_neighbor; a.q_background = q_background; a.contamination = contamination;
  a.contaminated = contaminated; a.total = total; a.percent = percent;
  const int Tp = (a.T + 3) & ~3;
  const size_t strips = (size_t)kContamWaves * Tp * sizeof(float);
  if (a.ld_s > 0) {
    // a workgroup pays for its copy of the table once and then walks rows: as many workgroups per CU as its LDS holds
    // copies of this table, at most the kMaxGroupsPerCu that its wave slots hold
    const size_t lds = (size_t)a.G_ref * a.ld_s * sizeof(float) + strips;
    int per_cu = (int)(kCuLdsBytes / lds);
    per_cu = per_cu < 1 ? 1 : per_cu > kMaxGroupsPerCu ? kMaxGroupsPerCu : per_cu;
    hipLaunchKernelGGL((contamination_posterior_kernel<true>), dim3((unsigned)contam_grid(n_rows, per_cu)), dim3(kContamThreads),
                       lds, stream, a);
  } else {
    hipLaunchKernelGGL((contamination_posterior_kernel<false>), dim3((unsigned)contam_grid(n_rows, 16)), dim3(kContamThreads),
                       strips, stream, a);
  }
  SEGGER_LAUNCH_CHECK("contamination_posterior_kernel");
  return SEGGER_OK;
}
