// What the GATv2 host layer (gatv2.hip: the C ABI, one plan per call) and its launchers share: the grid rule and the
// launchers' declarations.  The specialised launchers are instantiated per (pass, dtype) in translation units of their
// own (gatv2_inst.hip compiled with -DSEGGER_INST_PASS/-DSEGGER_INST_DTYPE) so the build parallelises.
#pragma once
#include "gatv2_kernels.h"

namespace segger {

enum class Pass : int { Fwd = 0, BwdDst = 1, BwdSrc = 2 };
// what one specialised launch runs: a pass of one edge type, or two edge types in one grid -- FwdPair: the forwards of `a`
// (group-per-row) and `b` (wave-per-row); BwdSrcDstPair: a's source pass and the one-pass destination pass of b (ditto)
enum class Kind : int { Fwd = 0, BwdDst = 1, BwdSrc = 2, FwdPair = 3, BwdSrcDstPair = 4 };

// destination rows walked per wave in the dst-side backward (amortises the per-block grad_att / grad_bias partial slab)
constexpr int kBwdRowIters = 8;
// ... but small graphs (tile batches of ~50 k nodes) keep one row batch per wave so the grid still has
// thousands of blocks: iterations grow with the row count, 1 below 32 k rows, 8 from 256 k rows up
static inline int bwd_row_iters(int64_t n_rows) {
  const int64_t it = n_rows / 32768;
  return (int)(it < 1 ? 1 : (it > kBwdRowIters ? kBwdRowIters : it));
}

// segger_gatv2_bwd_pair merges launches up to this many source rows of the two-pass edge type: every batch the entry
// points accept (they refuse 2^31 - 1 rows and more).  The environment variable of the same name overrides it (gatv2.hip)
#ifndef SEGGER_BWD_PAIR_MAX_ROWS
#define SEGGER_BWD_PAIR_MAX_ROWS 0x7fffffffLL
#endif

// (heads, channels/8) combinations with a specialised kernel
#define SEGGER_GEOMETRIES(X) \
  X(1, 4) X(2, 4) X(3, 4) X(4, 4) \
  X(1, 8) X(2, 8) X(3, 8) X(4, 8)

// ---- the grid rule: rows per block and blocks per launch of every pass, and with them the rows of the backward's slabs
// (the kernels write one slab row per block).  From this average degree on, the groups of a wave split ONE row (wave-per-row)
constexpr double kWavePerRowDegree = 32.0;
static inline bool use_wave_per_row(int64_t n_rows, int64_t n_edges) {
  return n_rows > 0 && (double)n_edges / (double)n_rows >= kWavePerRowDegree;
}

// groups per wave of a specialised geometry = rows a wave walks at a time in group-per-row mode
constexpr int wave_groups(int heads, int channels) {
  int gs = 1;
  while (gs < heads * channels / 8) gs *= 2;
  return 64 / gs;
}
#define X(H, LPH) static_assert(wave_groups(H, LPH * 8) == Geo<H, LPH>::NG, "the grid rule and the kernels disagree");
SEGGER_GEOMETRIES(X)
#undef X

struct Grid { int64_t rows_per_block, nblocks, nblocks_padded; };

// four waves per block; a wave walks one row (wave-per-row; the generic kernels always do) or one per group, and the
// specialised destination pass `dst_row_iters` such batches
static inline Grid gatv2_grid(Pass pass, int heads, int channels, bool wave_per_row, int dst_row_iters, int64_t n_rows) {
  Grid g;
  g.rows_per_block = 4 * (int64_t)(wave_per_row ? 1 : wave_groups(heads, channels)) * (pass == Pass::BwdDst ? dst_row_iters : 1);
  g.nblocks = (n_rows + g.rows_per_block - 1) / g.rows_per_block;
  g.nblocks_padded = pad_to_xcd(g.nblocks);
  return g;
}

// ---- launchers: they take parameters whose block counts are set, choose the template instance and launch ------------
// one per (kind, storage type), each defined by the gatv2_inst.hip slice of its pass and type; the order is the table's
#define SEGGER_GAT_LAUNCHERS(X)                                       \
  X(fwd, f32) X(fwd, bf16) X(fwd, f16)                                \
  X(bwd_dst, f32) X(bwd_dst, bf16) X(bwd_dst, f16)                    \
  X(bwd_src, f32) X(bwd_src, bf16) X(bwd_src, f16)                    \
  X(fwd_pair, f32) X(fwd_pair, bf16) X(fwd_pair, f16)                 \
  X(bwd_src_dst_pair, f32) X(bwd_src_dst_pair, bf16) X(bwd_src_dst_pair, f16)
static_assert(SEGGER_F32 == 0 && SEGGER_BF16 == 1 && SEGGER_F16 == 2, "the launcher table is indexed by the dtype code");

// `b`: the second edge type of the pair kinds (which have their modes fixed); NULL for the others
typedef int (*gat_launch_fn)(const GatParams& a, const GatParams* b, int heads, int channels, bool wave_per_row, hipStream_t stream);
#define X(kind, t) \
  int gatv2_launch_##kind##_##t(const GatParams& a, const GatParams* b, int heads, int channels, bool wave_per_row, hipStream_t stream);
SEGGER_GAT_LAUNCHERS(X)
#undef X

// `dtype` is one of the three codes (the plan has checked it)
static inline int launch_specialised(Kind kind, int dtype, const GatParams& a, const GatParams* b, int heads, int channels,
                                     bool wave_per_row, hipStream_t stream) {
#define X(kind, t) gatv2_launch_##kind##_##t,
  static const gat_launch_fn table[] = {SEGGER_GAT_LAUNCHERS(X)};
#undef X
  return table[(int)kind * 3 + dtype](a, b, heads, channels, wave_per_row, stream);
}

// any other (heads, channels <= 512), gatv2_generic.hip: its destination pass sums grad_att / grad_bias itself
bool gatv2_has_specialised(int heads, int channels);
int gatv2_launch_generic(Pass pass, const GatParams& p, int dtype, int heads, int channels, float* grad_att, float* grad_bias,
                         hipStream_t stream);

}  // namespace segger
