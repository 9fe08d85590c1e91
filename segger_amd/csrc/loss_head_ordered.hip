// The ordered backward of the one-launch loss head: every byte of grad_tx, grad_bd and the losses is a function of the
// inputs alone (the embeddings, the sampled indices, the weights, the incoming gradient) -- not of the scheduling, the
// grid or the order in which an atomic landed.  No float atomic (the radix sort's integer atomics cannot show in a keys-only
// result): loss_head.hip's route threads a
// row's contributions into a chain in the order its exchanges happened and adds hot rows and the whole boundary side with
// fp32 atomics; here the contributions are SORTED by (target row, role, contributor id) and every row walks its segment.
//
//   forward   segger_loss_head_fwd's loss kernel and finish, unchanged (their partial sums are added in a fixed order:
//             one partial per block, written by one thread from four wave sums, then strided sums of one workgroup --
//             also with DEFER_FINISH, where the same body runs in the backward launch), asked for no chains; then
//             keys     one key per possible contribution: 2 per loss_tx triplet (its positive's row, its negative's), 2 per
//                      loss_bd node, 1 per segmentation triplet (its sampled negative); an inactive / skipped one gets
//                      the row past the last.  key = row << (id_bits + 2) | role << id_bits | id, transcript rows first,
//                      boundary row j as n_tx + j.  The loss_tx range also leaves 1/d(t,p), 1/d(t,n) in tx_w.
//             sort     one keys-only radix sort over exactly the key's bits (sort_config.h: no scratch).
//             offsets  seg[r] = the first key of row r or above: a binary search per row.
//   backward  one grid, two block ranges: transcript ROWS (64 a block, a 16-lane group each) | one workgroup per boundary.
//             THE ORDER (include/segger_amd.h and DESIGN.md state it; tests/loss_head_ordered_cases.py is its oracle):
//             transcript row r = (1) its anchor term of loss_tx, + (2) the terms of the triplets naming r as positive, by
//               ascending triplet, + (3) as negative, by ascending triplet, + (4) the anchor term of its segmentation
//               triplet; fp32, rounded once, then the row normalisation's backward.  A row with at most kSerialCap
//               contributions under (2)-(3) adds them one after the other onto (1).  A longer row is summed by the whole
//               workgroup after the block's short rows: contribution k of the segment goes to partial sum k mod 16 (each
//               starts at zero and adds in segment order), and the row is (1) + P_0 + ... + P_15 + (4) in that order.
//             boundary row j = (1) its anchor term of loss_bd + P_0 + ... + P_15, where the partial sums take, k mod 16
//               again, first the row's sorted segment -- (2) loss_bd positives by ascending node, (3) loss_bd negatives
//               by ascending node, (4) sampled loss_sg negatives by ascending triplet -- and then, counting from zero
//               again, (5) its own loss_sg positives in the order of sg_pos_indptr / sg_pos_eid.
//             Which form a row takes depends on its segment's length, a function of the indices: the order is total.
//             Every loop is bounded by the number of keys whatever the buffers hold, every id read from a key is checked
//             against its matrix: a stale workspace gives wrong numbers, never a spinning kernel or a stray access.
//
// Row layout as loss_head.hip: 16 lanes per row, CPL = C / 16 consecutive channels per lane (C in {32, 64, 128}).
#include "common.h"
#include "post_common.h"
#include "sort_config.h"
#include "loss_head.h"

namespace segger {
namespace {

constexpr int kSerialCap = 64;                     // contributions a row's own lane group adds one after the other
constexpr int kTeam = 16;                          // lane groups of a workgroup = partial sums of a long row
constexpr int kOffsetThreads = 256;

struct OrderedParams {
  unsigned long long* keys_in;                     // [n_keys] as built, position = 2 t + role | 2 n_tx + 2 i + role | 2 n_tx + 2 n_bd + e
  const unsigned long long* keys;                  // [n_keys] sorted
  int32_t* seg;                                    // [n_tx + n_bd + 1]: first key of row r or above
  int64_t n_keys;
  int id_bits;                                     // key = row << (id_bits + 2) | role << id_bits | id
};

struct OrderedLayout {
  size_t keys_in, keys, seg, temp, total;
  size_t temp_bytes;
  int64_t n_keys, n_rows;
  int id_bits, key_bits;
};

OrderedLayout ordered_layout(int64_t n_tx, int64_t n_bd, int64_t n_sg) {
  OrderedLayout L;
  n_tx = n_tx > 0 ? n_tx : 0; n_bd = n_bd > 0 ? n_bd : 0; n_sg = n_sg > 0 ? n_sg : 0;
  const int64_t n_ids = n_tx > n_bd ? (n_tx > n_sg ? n_tx : n_sg) : (n_bd > n_sg ? n_bd : n_sg);
  L.n_keys = 2 * n_tx + 2 * n_bd + n_sg;
  L.n_rows = n_tx + n_bd;
  L.id_bits = bit_length((unsigned long long)n_ids);
  L.key_bits = L.id_bits + 2 + bit_length((unsigned long long)L.n_rows);       // (the row past the last included)
  Carver ws;
  (void)ws.take(segger_loss_head_workspace_bytes(n_tx, n_bd, n_sg));           // the forward's partial sums, first
  const size_t n = (size_t)(L.n_keys > 0 ? L.n_keys : 1);
  L.keys_in = ws.take(n * 8);
  L.keys = ws.take(n * 8);
  L.seg = ws.take((size_t)(L.n_rows + 1) * 4);
  size_t t = 0;
  unsigned long long* k64 = nullptr;
  (void)rocprim::radix_sort_keys<NoScratchSortConfig>(nullptr, t, k64, k64, n, 0, (unsigned)L.key_bits, (hipStream_t)0);
  L.temp_bytes = t;
  L.temp = ws.take(t > 0 ? t : 1);
  L.total = ws.total();
  return L;
}

// ------------------------------------------------------------------------------------------------------- keys ----
// The forward's three block ranges.  loss_tx: a 16-lane group per triplet (the distances again, as loss_head_fwd_kernel
// forms them); loss_bd nodes and loss_sg triplets: a thread each, no embedding is read.
template <typename T, int CPL>
__global__ __launch_bounds__(256) void loss_head_keys_kernel(LossHeadParams p, OrderedParams o) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane >> 4, gl = lane & 15, c0 = gl * CPL;
  const int blk = blockIdx.x;
  const int shift = o.id_bits + 2;
  const unsigned long long none = (unsigned long long)(p.n_tx + p.n_bd);       // the row past the last
  if (blk < p.nb_tx) {
    const T* ztx = static_cast<const T*>(p.ztx);
    const int64_t base = (int64_t)blk * kItemsPerBlock;
#pragma unroll 1
    for (int i = wave * 4 + grp; i < kItemsPerBlock; i += 16) {
      const int64_t t = base + i;
      bool ok = t < p.n_tx;                                      // group-uniform
      int64_t ip = ok ? p.tx_pos[t] : 0, in = ok ? p.tx_neg[t] : 0;
      if ((uint64_t)ip >= (uint64_t)p.n_tx || (uint64_t)in >= (uint64_t)p.n_tx) { ok = false; ip = in = 0; }
      const int64_t ia = ok ? t : 0;
      float a[CPL], pp[CPL], nn[CPL];
      Row<T, CPL>::load(ztx + ia * p.ld_ztx + c0, a);
      Row<T, CPL>::load(ztx + ip * p.ld_ztx + c0, pp);
      Row<T, CPL>::load(ztx + in * p.ld_ztx + c0, nn);
      float sp = 0.f, sn = 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const float dp = a[k] - pp[k] + p.tx_eps, dn = a[k] - nn[k] + p.tx_eps;
        sp = fmaf(dp, dp, sp); sn = fmaf(dn, dn, sn);
      }
      sp = lane_block_sum<16>(sp); sn = lane_block_sum<16>(sn);
      const float dap = sqrtf(sp), dan = sqrtf(sn);
      const bool active = ok && dap - dan + p.tx_margin > 0.f;
      if (t < p.n_tx && gl < 2) {                                  // lane 0: the positive's row, lane 1: the negative's
        const float d = gl == 0 ? dap : dan;
        const float wk = active && d > 0.f ? 1.0f / d : 0.f;
        const unsigned long long row = wk != 0.f ? (unsigned long long)(gl == 0 ? ip : in) : none;
        p.tx_w[2 * t + gl] = wk;
        o.keys_in[2 * t + gl] = (row << shift) | ((unsigned long long)gl << o.id_bits) | (unsigned long long)t;
      }
    }
  } else if (blk < p.nb_tx + p.nb_bd) {
    const int64_t i = (int64_t)(blk - p.nb_tx) * kItemsPerBlock + threadIdx.x;
    if (threadIdx.x < kItemsPerBlock && i < p.n_bd) {
      const int64_t ip = p.bd_pos[i], in = p.bd_neg[i];
      const bool ok = (uint64_t)ip < (uint64_t)p.n_bd && (uint64_t)in < (uint64_t)p.n_bd && p.bd_w[i] != 0.f;
      const unsigned long long rp = ok ? (unsigned long long)(p.n_tx + ip) : none;
      const unsigned long long rn = ok ? (unsigned long long)(p.n_tx + in) : none;
      unsigned long long* k = o.keys_in + 2 * p.n_tx + 2 * i;
      k[0] = (rp << shift) | (unsigned long long)i;
      k[1] = (rn << shift) | (1ull << o.id_bits) | (unsigned long long)i;
    }
  } else {
    const int64_t e = (int64_t)(blk - p.nb_tx - p.nb_bd) * kItemsPerBlock + threadIdx.x;
    if (threadIdx.x < kItemsPerBlock && e < p.n_sg) {
      const int64_t ia = p.sg_src[e], ip = p.sg_pos[e], in = p.sg_neg[e];
      const bool ok = (uint64_t)ia < (uint64_t)p.n_tx && (uint64_t)ip < (uint64_t)p.n_bd && (uint64_t)in < (uint64_t)p.n_bd;
      const unsigned long long row = ok ? (unsigned long long)(p.n_tx + in) : none;
      o.keys_in[2 * p.n_tx + 2 * p.n_bd + e] = (row << shift) | (2ull << o.id_bits) | (unsigned long long)e;
    }
  }
}

// seg[r] = the number of sorted keys below row r, r = 0 .. n_rows: at most 32 halvings, whatever the keys hold
__global__ __launch_bounds__(kOffsetThreads) void loss_head_offsets_kernel(OrderedParams o, int64_t n_rows) {
  const int64_t r = (int64_t)blockIdx.x * kOffsetThreads + threadIdx.x;
  if (r > n_rows) return;
  const unsigned long long want = (unsigned long long)r << (o.id_bits + 2);
  int64_t lo = 0, hi = o.n_keys;
#pragma unroll 1
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (o.keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  o.seg[r] = (int32_t)lo;
}

// --------------------------------------------------------------------------------------------------- backward ----
template <typename T, int CPL>
__global__ __launch_bounds__(256) void loss_head_ordered_bwd_kernel(LossHeadParams p, OrderedParams o) {
  constexpr int C = 16 * CPL;
  __shared__ float part[kTeam][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane >> 4, gl = lane & 15, c0 = gl * CPL;
  const int team = wave * 4 + grp;                                // this lane group among the workgroup's 16
  const int blk = blockIdx.x;
  const T* ztx = static_cast<const T*>(p.ztx);
  const T* zbd = static_cast<const T*>(p.zbd);
  if (p.defer && blk == p.nb_tx + p.nb_sg) {                      // one extra workgroup: the forward's finishing launch, deferred
    loss_head_finish_body(p);
    return;
  }
  const unsigned long long id_mask = (1ull << o.id_bits) - 1ull;
  const float sc_sg = p.n_sg > 0 ? graw_of(p, 2) * (p.sg_kind == SEGGER_LOSS_BCE ? 0.5f : 1.0f) / (float)p.n_sg : 0.f;
  // the segment of row `row` (transcript r, or n_tx + j), clamped to the keys there are
  auto segment = [&](int64_t row, int64_t& beg, int64_t& end) {
    beg = o.seg[row]; end = o.seg[row + 1];
    if (beg < 0) beg = 0;
    if (end > o.n_keys) end = o.n_keys;
    if (end < beg) end = beg;
  };
  if (blk < p.nb_tx) {
    const float sc_tx = p.n_tx > 0 ? graw_of(p, 0) / (float)p.n_tx : 0.f;
    const int64_t base = (int64_t)blk * kItemsPerBlock;
    // the row's gradient through z = y / max(|y|, eps) when y is given (csrc/frontend.hip l2norm_kernel), then the store
    auto finish_row = [&](int64_t row, float (&g)[CPL]) {
      if (p.ytx != nullptr) {
        float y[CPL];
        Row<T, CPL>::load(static_cast<const T*>(p.ytx) + row * p.ld_ytx + c0, y);
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) ss = fmaf(y[k], y[k], ss);
        const float nrm = sqrtf(lane_block_sum<16>(ss));
        const float inv = 1.0f / fmaxf(nrm, p.norm_eps);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) dot = fmaf(y[k] * inv, g[k], dot);
        dot = lane_block_sum<16>(dot);
        if (nrm < p.norm_eps) dot = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) g[k] = (g[k] - y[k] * inv * dot) * inv;
      }
      Row<T, CPL>::store(static_cast<T*>(p.gtx) + row * p.ld_gtx + c0, g);
    };
    // (1) g = the anchor term of row r's own loss_tx triplet
    auto anchor_tx = [&](int64_t r, const float (&a)[CPL], float (&g)[CPL]) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) g[k] = 0.f;
      const float wp = p.tx_w[2 * r] * sc_tx, wn = p.tx_w[2 * r + 1] * sc_tx;
      const int64_t ip = p.tx_pos[r], in = p.tx_neg[r];
      if ((p.tx_w[2 * r] != 0.f || p.tx_w[2 * r + 1] != 0.f) && (uint64_t)ip < (uint64_t)p.n_tx && (uint64_t)in < (uint64_t)p.n_tx) {
        float pp[CPL], nn[CPL];
        Row<T, CPL>::load(ztx + ip * p.ld_ztx + c0, pp);
        Row<T, CPL>::load(ztx + in * p.ld_ztx + c0, nn);
#pragma unroll
        for (int k = 0; k < CPL; ++k) g[k] += (a[k] - pp[k] + p.tx_eps) * wp - (a[k] - nn[k] + p.tx_eps) * wn;
      }
    };
    // (2), (3): g += the terms of the keys first, first + step, ... below end (role 0: r is the triplet's positive)
    auto walk_tx = [&](const float (&a)[CPL], float (&g)[CPL], int64_t first, int64_t end, int step) {
      // kAhead terms in flight: their keys, then their weights and rows, are loaded together (a term's loads depend on
      // its key, one term on no other), and they are ADDED one after the other in list order -- the sum's order is the
      // loop's without the batching
      constexpr int kAhead = 4;
#pragma unroll 1
      for (int64_t k = first; k < end; k += (int64_t)kAhead * step) {
        int64_t t[kAhead];
        int role[kAhead];
        bool ok[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const int64_t ku = k + (int64_t)u * step;
          const unsigned long long key = ku < end ? o.keys[ku] : ~0ull;
          t[u] = (int64_t)(key & id_mask);
          role[u] = (int)(key >> o.id_bits) & 1;
          ok[u] = ku < end && t[u] < p.n_tx;
          if (!ok[u]) t[u] = 0;
        }
        float w[kAhead], at[kAhead][CPL];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          w[u] = p.tx_w[2 * t[u] + role[u]] * sc_tx;
          Row<T, CPL>::load(ztx + t[u] * p.ld_ztx + c0, at[u]);
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          if (!ok[u]) continue;                                    // group-uniform
          const float sgn = role[u] ? w[u] : -w[u];
#pragma unroll
          for (int k2 = 0; k2 < CPL; ++k2) g[k2] = fmaf(at[u][k2] - a[k2] + p.tx_eps, sgn, g[k2]);
        }
      }
    };
    // (4) g += the anchor term of the row's segmentation triplet (a transcript lies in at most one boundary)
    auto anchor_sg = [&](int64_t r, const float (&a)[CPL], float (&g)[CPL]) {
      if (p.sg_of_tx == nullptr || sc_sg == 0.f) return;
      const int64_t e = p.sg_of_tx[r];
      if (e < 0 || e >= p.n_sg) return;
      const int64_t j = p.sg_pos[e], jn = p.sg_neg[e];
      if (p.sg_src[e] != r || (uint64_t)j >= (uint64_t)p.n_bd || (uint64_t)jn >= (uint64_t)p.n_bd) return;
      float pj[CPL], nv[CPL];
      Row<T, CPL>::load(zbd + j * p.ld_zbd + c0, pj);
      Row<T, CPL>::load(zbd + jn * p.ld_zbd + c0, nv);
      float s0 = 0.f, s1 = 0.f;
      if (p.sg_kind == SEGGER_LOSS_BCE) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) { s0 = fmaf(a[k], pj[k], s0); s1 = fmaf(a[k], nv[k], s1); }
        s0 = lane_block_sum<16>(s0); s1 = lane_block_sum<16>(s1);
        const float dlp = (sigmoid(s0) - 1.0f) * sc_sg, dln = sigmoid(s1) * sc_sg;
#pragma unroll
        for (int k = 0; k < CPL; ++k) g[k] += dlp * pj[k] + dln * nv[k];
      } else {
        float dp[CPL], dn[CPL];
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          dp[k] = a[k] - pj[k] + p.sg_eps; dn[k] = a[k] - nv[k] + p.sg_eps;
          s0 = fmaf(dp[k], dp[k], s0); s1 = fmaf(dn[k], dn[k], s1);
        }
        s0 = lane_block_sum<16>(s0); s1 = lane_block_sum<16>(s1);
        const float dap = sqrtf(s0), dan = sqrtf(s1);
        if (dap - dan + p.sg_margin > 0.f) {
          const float ip_ = dap > 0.f ? sc_sg / dap : 0.f, in_ = dan > 0.f ? sc_sg / dan : 0.f;
#pragma unroll
          for (int k = 0; k < CPL; ++k) g[k] += dp[k] * ip_ - dn[k] * in_;
        }
      }
    };
    // ---- short rows: one per 16-lane group, everything in registers, stored once
#pragma unroll 1
    for (int i = team; i < kItemsPerBlock; i += kTeam) {
      const int64_t r = base + i;
      if (r >= p.n_tx) continue;                                   // group-uniform
      int64_t beg, end;
      segment(r, beg, end);
      if (end - beg > kSerialCap) continue;                        // a long row: the workgroup's, below
      float a[CPL], g[CPL];
      Row<T, CPL>::load(ztx + r * p.ld_ztx + c0, a);
      anchor_tx(r, a, g);
      walk_tx(a, g, beg, end, 1);
      anchor_sg(r, a, g);
      finish_row(r, g);
    }
    // ---- long rows: 16 interleaved partial sums, added onto the anchor term in ascending order (all branches are
    // workgroup-uniform: the segment's bounds are the same word for every thread)
#pragma unroll 1
    for (int i = 0; i < kItemsPerBlock; ++i) {
      const int64_t r = base + i;
      if (r >= p.n_tx) break;
      int64_t beg, end;
      segment(r, beg, end);
      if (end - beg <= kSerialCap) continue;
      float a[CPL], g[CPL];
      Row<T, CPL>::load(ztx + r * p.ld_ztx + c0, a);
#pragma unroll
      for (int k = 0; k < CPL; ++k) g[k] = 0.f;
      walk_tx(a, g, beg + team, end, kTeam);
#pragma unroll
      for (int k = 0; k < CPL; ++k) part[team][c0 + k] = g[k];
      __syncthreads();
      if (team == 0) {
        anchor_tx(r, a, g);
#pragma unroll 1
        for (int q = 0; q < kTeam; ++q) {
#pragma unroll
          for (int k = 0; k < CPL; ++k) g[k] += part[q][c0 + k];
        }
        anchor_sg(r, a, g);
        finish_row(r, g);
      }
      __syncthreads();                                             // the partial sums are rewritten by the next long row
    }
    return;
  }
  // ---- one boundary row per workgroup
  const int64_t j = blk - p.nb_tx;
  if (j >= p.n_bd) return;
  const float sc_bd = graw_of(p, 1);
  float x[CPL], acc[CPL];
  Row<T, CPL>::load(zbd + j * p.ld_zbd + c0, x);
  float sjj = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k) { sjj = fmaf(x[k], x[k], sjj); acc[k] = 0.f; }
  sjj = lane_block_sum<16>(sjj);
  const float nj = sqrtf(sjj), cj = fmaxf(nj, p.bd_eps);
  int64_t beg, end;
  segment(p.n_tx + j, beg, end);
  // (2), (3), (4): the sorted segment, contribution k to lane group k mod 16
#pragma unroll 1
  for (int64_t s = beg + team; s < end; s += kTeam) {
    const unsigned long long key = o.keys[s];
    const int64_t id = (int64_t)(key & id_mask);
    const int role = (int)(key >> o.id_bits) & 3;
    if (role < 2) {
      // node `id` of loss_bd names j as its positive (role 0) or negative (role 1): csrc/heads.hip metric_kernel's terms
      if (id >= p.n_bd) continue;
      const float w = p.bd_w[id], d = role ? p.bd_dneg[id] : p.bd_dpos[id];
      float xi[CPL];
      Row<T, CPL>::load(zbd + id * p.ld_zbd + c0, xi);
      float sxx = 0.f, sxy = 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) { sxx = fmaf(xi[k], xi[k], sxx); sxy = fmaf(xi[k], x[k], sxy); }
      sxx = lane_block_sum<16>(sxx); sxy = lane_block_sum<16>(sxy);
      const float cx = fmaxf(sqrtf(sxx), p.bd_eps);
      const float cosv = sxy / (cx * cj);
      const float gq = 2.f * w * (cosv - (1.f - d)) * sc_bd;
      const float iq = gq / (cx * cj), bq = nj > p.bd_eps ? gq * cosv / sjj : 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] += iq * xi[k] - bq * x[k];
    } else {
      // segmentation triplet `id` drew j as its negative
      if (id >= p.n_sg) continue;
      const int64_t ia = p.sg_src[id], ip = p.sg_pos[id];
      if ((uint64_t)ia >= (uint64_t)p.n_tx || (uint64_t)ip >= (uint64_t)p.n_bd) continue;
      float a[CPL];
      Row<T, CPL>::load(ztx + ia * p.ld_ztx + c0, a);
      if (p.sg_kind == SEGGER_LOSS_BCE) {
        float s1 = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) s1 = fmaf(a[k], x[k], s1);
        s1 = lane_block_sum<16>(s1);
        const float dln = sigmoid(s1) * sc_sg;
#pragma unroll
        for (int k = 0; k < CPL; ++k) acc[k] = fmaf(dln, a[k], acc[k]);
      } else {
        float pp[CPL], dn[CPL];
        Row<T, CPL>::load(zbd + ip * p.ld_zbd + c0, pp);
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const float dp = a[k] - pp[k] + p.sg_eps;
          dn[k] = a[k] - x[k] + p.sg_eps;
          s0 = fmaf(dp, dp, s0); s1 = fmaf(dn[k], dn[k], s1);
        }
        s0 = lane_block_sum<16>(s0); s1 = lane_block_sum<16>(s1);
        const float dap = sqrtf(s0), dan = sqrtf(s1);
        if (dap - dan + p.sg_margin > 0.f) {
          const float in_ = dan > 0.f ? sc_sg / dan : 0.f;
#pragma unroll
          for (int k = 0; k < CPL; ++k) acc[k] += dn[k] * in_;
        }
      }
    }
  }
  // (5): the boundary's own segmentation triplets, in the order of their grouping by positive row
  if (p.n_sg > 0) {
    int64_t sb = p.sg_indptr[j], se = p.sg_indptr[j + 1];
    if (sb < 0) sb = 0;
    if (se > p.n_sg) se = p.n_sg;
#pragma unroll 1
    for (int64_t s = sb + team; s < se; s += kTeam) {
      const int64_t e = (int64_t)p.sg_eid[s];
      if ((uint64_t)e >= (uint64_t)p.n_sg) continue;
      const int64_t ia = p.sg_src[e], in = p.sg_neg[e];
      if (p.sg_pos[e] != j || (uint64_t)ia >= (uint64_t)p.n_tx || (uint64_t)in >= (uint64_t)p.n_bd) continue;
      float a[CPL];
      Row<T, CPL>::load(ztx + ia * p.ld_ztx + c0, a);
      if (p.sg_kind == SEGGER_LOSS_BCE) {
        float s0 = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) s0 = fmaf(a[k], x[k], s0);
        s0 = lane_block_sum<16>(s0);
        const float dlp = (sigmoid(s0) - 1.0f) * sc_sg;
#pragma unroll
        for (int k = 0; k < CPL; ++k) acc[k] = fmaf(dlp, a[k], acc[k]);
      } else {
        float nv[CPL], dp[CPL];
        Row<T, CPL>::load(zbd + in * p.ld_zbd + c0, nv);
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          dp[k] = a[k] - x[k] + p.sg_eps;
          const float dn = a[k] - nv[k] + p.sg_eps;
          s0 = fmaf(dp[k], dp[k], s0); s1 = fmaf(dn, dn, s1);
        }
        s0 = lane_block_sum<16>(s0); s1 = lane_block_sum<16>(s1);
        const float dap = sqrtf(s0), dan = sqrtf(s1);
        if (dap - dan + p.sg_margin > 0.f) {
          const float ip_ = dap > 0.f ? sc_sg / dap : 0.f;
#pragma unroll
          for (int k = 0; k < CPL; ++k) acc[k] -= dp[k] * ip_;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CPL; ++k) part[team][c0 + k] = acc[k];
  __syncthreads();
  if (team != 0) return;
  // (1): the row's own loss_bd term, then the 16 partial sums in ascending order, one store
  float g[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) g[k] = 0.f;
  {
    const int64_t ip = p.bd_pos[j], in = p.bd_neg[j];
    const float w = p.bd_w[j];
    if ((uint64_t)ip < (uint64_t)p.n_bd && (uint64_t)in < (uint64_t)p.n_bd && w != 0.f) {
      float yp[CPL], yn[CPL];
      Row<T, CPL>::load(zbd + ip * p.ld_zbd + c0, yp);
      Row<T, CPL>::load(zbd + in * p.ld_zbd + c0, yn);
      float spp = 0.f, snn = 0.f, sxp = 0.f, sxn = 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        spp = fmaf(yp[k], yp[k], spp); snn = fmaf(yn[k], yn[k], snn);
        sxp = fmaf(x[k], yp[k], sxp); sxn = fmaf(x[k], yn[k], sxn);
      }
      spp = lane_block_sum<16>(spp); snn = lane_block_sum<16>(snn);
      sxp = lane_block_sum<16>(sxp); sxn = lane_block_sum<16>(sxn);
      const float cp = fmaxf(sqrtf(spp), p.bd_eps), cn = fmaxf(sqrtf(snn), p.bd_eps);
      const float cos_p = sxp / (cj * cp), cos_n = sxn / (cj * cn);
      const float gp = 2.f * w * (cos_p - (1.f - p.bd_dpos[j])) * sc_bd, gn = 2.f * w * (cos_n - (1.f - p.bd_dneg[j])) * sc_bd;
      const float ax = nj > p.bd_eps ? (gp * cos_p + gn * cos_n) / sjj : 0.f;
      const float ip_ = gp / (cj * cp), in_ = gn / (cj * cn);
#pragma unroll
      for (int k = 0; k < CPL; ++k) g[k] = ip_ * yp[k] + in_ * yn[k] - ax * x[k];
    }
  }
#pragma unroll 1
  for (int q = 0; q < kTeam; ++q) {
#pragma unroll
    for (int k = 0; k < CPL; ++k) g[k] += part[q][c0 + k];
  }
  Row<float, CPL>::store(p.gbd + j * C + c0, g);
}

int fill_ordered(const segger_loss_head_args* a, bool bwd, const char* who, LossHeadParams* out, OrderedParams* ord, OrderedLayout* lay) {
  SEGGER_REQUIRE(a != nullptr, "%s: args is NULL", who);
  SEGGER_REQUIRE(a->n_tx >= 0 && a->n_bd >= 0 && a->n_sg >= 0, "%s: negative size", who);
  SEGGER_REQUIRE(a->channels == 32 || a->channels == 64 || a->channels == 128, "%s: channels must be 32, 64 or 128", who);
  SEGGER_REQUIRE(a->dtype == SEGGER_F32 || a->dtype == SEGGER_BF16 || a->dtype == SEGGER_F16, "%s: unknown dtype %d", who, a->dtype);
  SEGGER_REQUIRE(a->n_tx < 0x1fffffffLL && a->n_bd < 0x1fffffffLL && a->n_sg < 0x1fffffffLL, "%s: batch too large", who);
  const size_t es = esize(a->dtype);
  const size_t row_align = (size_t)(a->channels / 16) * es >= 16 ? 16 : (size_t)(a->channels / 16) * es;
  SEGGER_REQUIRE(a->n_tx == 0 || (a->z_tx && ((uintptr_t)a->z_tx % 16) == 0 && ((size_t)a->ld_ztx * es) % row_align == 0 && a->ld_ztx >= a->channels),
                 "%s: z_tx NULL, misaligned or ld < channels", who);
  SEGGER_REQUIRE(a->n_bd == 0 || (a->z_bd && ((uintptr_t)a->z_bd % 16) == 0 && ((size_t)a->ld_zbd * es) % row_align == 0 && a->ld_zbd >= a->channels),
                 "%s: z_bd NULL, misaligned or ld < channels", who);
  SEGGER_REQUIRE(a->n_tx == 0 || (a->tx_pos && a->tx_neg), "%s: NULL loss_tx triplets", who);
  SEGGER_REQUIRE(a->n_bd == 0 || (a->bd_pos && a->bd_neg && a->bd_dpos && a->bd_dneg && a->bd_w), "%s: NULL loss_bd input", who);
  SEGGER_REQUIRE(a->n_sg == 0 || (a->sg_src && a->sg_pos && a->sg_neg), "%s: NULL loss_sg triplets", who);
  SEGGER_REQUIRE(a->sg_kind == SEGGER_LOSS_TRIPLET || a->sg_kind == SEGGER_LOSS_BCE, "%s: unknown sg_kind", who);
  SEGGER_REQUIRE(a->a && a->b && a->out, "%s: NULL a / b / out", who);
  SEGGER_REQUIRE(!a->tx_state && !a->tx_next && !a->tx_hot_id && !a->tx_hot_acc, "%s: the ordered route keeps no chains: tx_state, tx_next, tx_hot_id and tx_hot_acc must be NULL", who);
  const OrderedLayout L = ordered_layout(a->n_tx, a->n_bd, a->n_sg);
  SEGGER_REQUIRE(L.n_keys < 0x7fffffffLL, "%s: batch too large", who);
  SEGGER_REQUIRE(a->workspace && is_aligned(a->workspace, 256), "%s: workspace NULL or not 256-byte aligned", who);
  if (a->workspace_bytes < L.total) return workspace_too_small(who, a->workspace_bytes, L.total);
  LossHeadParams p{};
  p.ztx = a->z_tx; p.ld_ztx = a->ld_ztx; p.n_tx = a->n_tx;
  p.zbd = a->z_bd; p.ld_zbd = a->ld_zbd; p.n_bd = a->n_bd;
  p.tx_pos = a->tx_pos; p.tx_neg = a->tx_neg; p.tx_margin = a->tx_margin; p.tx_eps = a->tx_eps;
  p.bd_pos = a->bd_pos; p.bd_neg = a->bd_neg; p.bd_dpos = a->bd_dpos; p.bd_dneg = a->bd_dneg; p.bd_w = a->bd_w; p.bd_eps = a->bd_eps;
  p.sg_src = a->sg_src; p.sg_pos = a->sg_pos; p.sg_neg = a->sg_neg; p.n_sg = a->n_sg;
  p.sg_margin = a->sg_margin; p.sg_eps = a->sg_eps; p.sg_kind = a->sg_kind;
  p.sg_indptr = a->sg_pos_indptr; p.sg_eid = a->sg_pos_eid; p.sg_of_tx = a->sg_of_tx;
  p.a = a->a; p.b = a->b; p.gout = a->grad_out; p.out = a->out; p.graw = a->grad_raw;
  p.tx_w = a->tx_w;
  p.ytx = a->y_tx; p.ld_ytx = a->ld_ytx; p.norm_eps = a->norm_eps;
  p.gtx = a->grad_tx; p.ld_gtx = a->ld_gtx; p.gbd = a->grad_bd;
  p.partial = static_cast<float*>(a->workspace);
  p.nb_tx = (int)blocks_of(a->n_tx); p.nb_bd = (int)blocks_of(a->n_bd); p.nb_sg_fin = (int)blocks_of(a->n_sg);
  p.nb_sg = (int)a->n_bd;                                         // the backward: one workgroup per boundary
  p.defer = (a->reserved_ & SEGGER_LOSS_HEAD_DEFER_FINISH) ? 1 : 0;
  SEGGER_REQUIRE(!p.defer || a->grad_out, "%s: DEFER_FINISH needs grad_out (the gradient the backward will receive)", who);
  if (bwd) {
    SEGGER_REQUIRE(a->tx_w && (p.defer || a->grad_raw), "%s: needs the forward's tx_w and grad_raw", who);
    SEGGER_REQUIRE(a->n_tx == 0 || (a->grad_tx && ((uintptr_t)a->grad_tx % 16) == 0 && ((size_t)a->ld_gtx * es) % row_align == 0 && a->ld_gtx >= a->channels),
                   "%s: grad_tx NULL, misaligned or ld < channels", who);
    SEGGER_REQUIRE(a->n_bd == 0 || (a->grad_bd && is_aligned(a->grad_bd, 16)), "%s: grad_bd NULL or not 16-byte aligned", who);
    SEGGER_REQUIRE(!a->y_tx || (((uintptr_t)a->y_tx % 16) == 0 && ((size_t)a->ld_ytx * es) % row_align == 0 && a->ld_ytx >= a->channels),
                   "%s: y_tx misaligned or ld < channels", who);
    SEGGER_REQUIRE(a->n_sg == 0 || (a->sg_pos_indptr && a->sg_pos_eid), "%s: the segmentation triplets need their grouping by positive row", who);
  }
  OrderedParams o{};
  o.keys_in = at<unsigned long long>(a->workspace, L.keys_in);
  o.keys = at<unsigned long long>(a->workspace, L.keys);
  o.seg = at<int32_t>(a->workspace, L.seg);
  o.n_keys = L.n_keys;
  o.id_bits = L.id_bits;
  *out = p; *ord = o; *lay = L;
  return SEGGER_OK;
}

template <typename F>
int with_row_type(const segger_loss_head_args* a, const char* who, F&& f) {
  return dispatch_dtype(a->dtype, who, [&](auto t) -> int {
    if (a->channels == 32) f(t, int_c<2>{}); else if (a->channels == 64) f(t, int_c<4>{}); else f(t, int_c<8>{});
    return SEGGER_OK;
  });
}

}  // namespace
}  // namespace segger

using namespace segger;

extern "C" size_t segger_loss_head_ordered_workspace_bytes(int64_t n_tx, int64_t n_bd, int64_t n_sg) {
  return ordered_layout(n_tx, n_bd, n_sg).total;
}

extern "C" int segger_loss_head_ordered_fwd(const segger_loss_head_args* a, segger_stream_t stream_) {
  const char* who = "segger_loss_head_ordered_fwd";
  hipStream_t stream = (hipStream_t)stream_;
  LossHeadParams p;
  OrderedParams o;
  OrderedLayout L;
  int rc = fill_ordered(a, false, who, &p, &o, &L);
  if (rc != SEGGER_OK) return rc;
  // the losses (and, without DEFER_FINISH, their finish): the chained route's forward, asked for no chains and no fill
  segger_loss_head_args f = *a;
  f.tx_w = nullptr;
  f.grad_bd = nullptr;
  rc = segger_loss_head_fwd(&f, stream_);
  if (rc != SEGGER_OK || a->tx_w == nullptr || L.n_keys == 0) return rc;
  const int64_t grid = (int64_t)p.nb_tx + p.nb_bd + p.nb_sg_fin;
  rc = with_row_type(a, who, [&](auto t, auto cpl) {
    hipLaunchKernelGGL((loss_head_keys_kernel<elem_t<decltype(t)>, decltype(cpl)::value>), dim3((unsigned)grid), dim3(256), 0, stream, p, o);
  });
  if (rc != SEGGER_OK) return rc;
  SEGGER_LAUNCH_CHECK("loss_head_keys_kernel");
  size_t temp_bytes = L.temp_bytes;
  SEGGER_HIP(rocprim::radix_sort_keys<NoScratchSortConfig>(at<char>(a->workspace, L.temp), temp_bytes, o.keys_in,
                                                           const_cast<unsigned long long*>(o.keys), (size_t)L.n_keys, 0,
                                                           (unsigned)L.key_bits, stream));
  hipLaunchKernelGGL(loss_head_offsets_kernel, dim3((unsigned)ceil_div(L.n_rows + 1, kOffsetThreads)), dim3(kOffsetThreads), 0,
                     stream, o, L.n_rows);
  SEGGER_LAUNCH_CHECK("loss_head_offsets_kernel");
  return SEGGER_OK;
}

extern "C" int segger_loss_head_ordered_bwd(const segger_loss_head_args* a, segger_stream_t stream_) {
  const char* who = "segger_loss_head_ordered_bwd";
  hipStream_t stream = (hipStream_t)stream_;
  LossHeadParams p;
  OrderedParams o;
  OrderedLayout L;
  int rc = fill_ordered(a, true, who, &p, &o, &L);
  if (rc != SEGGER_OK) return rc;
  const int64_t grid = (int64_t)p.nb_tx + p.nb_sg + (p.defer ? 1 : 0);
  if (grid == 0) return SEGGER_OK;
  rc = with_row_type(a, who, [&](auto t, auto cpl) {
    hipLaunchKernelGGL((loss_head_ordered_bwd_kernel<elem_t<decltype(t)>, decltype(cpl)::value>), dim3((unsigned)grid), dim3(256), 0, stream, p, o);
  });
  if (rc != SEGGER_OK) return rc;
  SEGGER_LAUNCH_CHECK("loss_head_ordered_bwd_kernel");
  return SEGGER_OK;
}
