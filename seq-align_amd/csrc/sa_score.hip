// sa_score.hip -- score only: the optimal score of each pair, no matrices, no traceback, any length.
//
// The same row sweep as every fill (sa_rowsweep.hpp: one row per step in registers, the (max,+) scan for gap_b, the
// GENERAL path for the reference's flags), with the stores taken out.  What is kept instead:
//   NW  nothing per cell: after the last row a lane's X[c] IS max(match, gap_a, gap_b) of its cell on that row, and the
//       reference's end pick (needleman_wunsch.c:54-66) is the largest of the three at (len_a, len_b) -- no_end_gap_penalty
//       is inside RowSweep's last row and column, so the score comes out of the same cells;
//   SW  per column the highest match_scores value and the first row that reached it (strict >: a tie keeps the lower row),
//       reduced at the end in hit order -- score desc, column asc, row asc (smith_waterman.c:71-86).
//
// score_rows_kernel: rows of up to 1 024 columns, one wave per pair (CPL = 1..16 columns per lane), 4 pairs per
// workgroup.  len_b is unlimited: seq_b's codes arrive 64 rows at a time, the left border column is arithmetic.
// Its CROSS form (seqalign_*_score_cross, kind "score_cross") takes a query and a target of two sets instead of a pair of
// a list: same sweep, same end picks, only which sequences a wave reads and where its result goes differ.
//
// score_strips_kernel: wider rows, the strips pipeline (sa_strips.hpp) -- but what strip s hands strip s + 1 is not the
// matrices: the hand-off column (StripHandoff), O(strips x len_b) bytes per pair.  SW: each strip merges its best cell into
// the best of the strips to its left and hands that on; the last strip writes the pair's result.  Cell indices and the
// error key are 64-bit (len_a x len_b may pass 2^32).
#include "sa_strips.hpp"

namespace sa {

constexpr int kScoreStripCPL = 8;                            // 512 columns per strip, as sa_fill_strips.hip
constexpr uint32_t kScoreStripCols = kWave * kScoreStripCPL;

// CROSS: wave w of a launch for one row class takes target t_order[w / nq] and query q_list[w % nq].  t_order runs longest
// first; within a class a row costs the same whatever len_a is, so a wave's cost follows its target's length and the long
// ones start first.  That order is for speed only: which wave runs when decides no result.  The result goes to
// [q * n_t + t] of the tile; a failing pair leaves only its index, in one 64-bit atomicMin.
template <int CPL, int SUBST, bool GENERAL, bool SW, bool CROSS = false>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
score_rows_kernel(const std::conditional_t<CROSS, SaScoreCrossParams, SaScoreParams> kp) {
  const SaScoreParams &sp = sa_pair_params(kp);
  const SaFillParams &p = sp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t pair = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  uint32_t qa = pair, tb = pair;   // descriptors of seq_a and seq_b
  uint64_t at = pair;              // where the result goes
  if constexpr (CROSS) {
    if (pair >= kp.n_waves) return;   // wave-uniform, after the only barrier
    const uint32_t ti = pair / kp.nq;
    qa = kp.q_list[pair - ti * kp.nq];
    tb = kp.t_order[ti];
    at = (uint64_t)qa * kp.n_t + tb;
  } else {
    if (pair >= p.n_pairs) return;   // wave-uniform, after the only barrier
  }

  const uint32_t la = p.len_a[qa], lb = p.len_b[tb];
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[qa];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[tb];
  const uint32_t W = la + 1;

  const SweepConsts k(p, table);
  const Border bd{p.floor, p.gap_open, p.ext, SW, (p.flags & SA_F_NO_START_GAP) != 0};

  RowSweep<CPL, SUBST, GENERAL> sw;
  const uint32_t col0 = lane * CPL;
  const int ncol = max(0, min(CPL, (int)la - lane * CPL));
  sw.start_strip(p, k, bd, sa_, la, 0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  BestCells<SW ? CPL : 1> best;
  if constexpr (SW) best.init();

  int code = 0;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {   // every 64 rows: lane t fetches seq_b's code for row j + t
      const uint32_t r = j + lane;
      if (r <= lb) code = p.code[sb_[r - 1]];
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    // the border column (reference alignment.c:72-80): max(M, A) and B of cell (0, j)
    const int feedZ = max(k.floor_, bd.edge_gap(j)), feedB = k.floor_;
    int mv[CPL], av[CPL], bv[CPL];
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code, q), feedZ, feedB, mv, av, bv);
    if constexpr (SW) best.row(mv, j);
  }

  const unsigned long long err = sw.reduce_err();
  if constexpr (SW) {
    int score;
    unsigned long long key;
    best.reduce(col0, ncol, score, key);
    if (lane == 0) {
      sp.score[at] = score;
      sp.end_a[at] = score > 0 ? (uint32_t)(key >> 32) : 0u;
      sp.end_b[at] = score > 0 ? (uint32_t)key : 0u;
    }
  } else {
    if (la == 0) {   // cell (0, len_b) of the border column
      if (lane == 0) sp.score[at] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
    } else {
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (col0 + c + 1 == la) sp.score[at] = sw.X[c];   // max(M, A, B) of (len_a, len_b)
    }
  }
  if constexpr (CROSS) {
    if (lane == 0 && err != ~0ull) {
      atomicMin(kp.err_pair, (unsigned long long)at);
      atomicOr(sp.err_flag, 1u);
    }
  } else {
    if (lane == 0) {
      p.status[pair] = err;
      if (err != ~0ull) atomicOr(sp.err_flag, 1u);
    }
  }
}

template <int SUBST, bool GENERAL, bool SW>
__global__ void __launch_bounds__(kWave)
score_strips_kernel(const SaScoreParams sp) {
  constexpr int CPL = kScoreStripCPL;
  const SaFillParams &p = sp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x;
  const uint32_t spp = sp.strips_per_pair;
  uint32_t strip, pair;
  strip_of_ticket(strip_ticket(sp.progress + (uint64_t)gridDim.x), spp, strip, pair);
  if (pair >= p.n_pairs) return;

  const uint32_t la = p.len_a[pair], lb = p.len_b[pair];
  const uint32_t i0 = strip * kScoreStripCols;
  if (i0 >= la && strip != 0) return;   // this pair has fewer strips
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[pair];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[pair];
  const uint32_t W = la + 1;
  const uint64_t slot = (uint64_t)pair * spp + strip;   // my progress word / strip_best entry
  uint32_t *done = sp.progress + (uint64_t)pair * spp;  // done[s] = rows strip s has handed over
  const uint64_t rows = (uint64_t)lb + 1;
  int32_t *hand_out = sp.handoff + 2 * (sp.handoff_off[pair] + (uint64_t)strip * rows);
  const int32_t *hand_in = sp.handoff + 2 * (sp.handoff_off[pair] + (uint64_t)(strip ? strip - 1 : 0) * rows);

  const SweepConsts k(p, table);
  const Border bd{p.floor, p.gap_open, p.ext, SW, (p.flags & SA_F_NO_START_GAP) != 0};

  const uint32_t cols = (i0 < la) ? min(kScoreStripCols, la - i0) : 0;
  const bool last_strip = i0 + kScoreStripCols >= la;
  const uint32_t col0 = i0 + lane * CPL;
  const int ncol = max(0, min(CPL, (int)cols - lane * CPL));
  RowSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, bd, sa_, la, i0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  BestCells<SW ? CPL : 1> best;
  if constexpr (SW) best.init();

  StripHandoff h;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {
      // rows j .. j + 63 of the strip to my left must have been handed over
      if (strip > 0) strip_wait(done + strip - 1, min(j + kWave - 1, lb));
      h.load(p, k, bd, sb_, lb, strip, hand_in, j + lane);
    }
    int mv[CPL], av[CPL], bv[CPL];
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(h.code, q), read_lane(h.fz, q), read_lane(h.fb, q), mv, av, bv);
    if constexpr (SW) best.row(mv, j);
    if (!last_strip) {   // StripHandoff::keep, open-coded: through the helper this kernel's SGPR counts and spills move
      const int z = read_lane(max(mv[CPL - 1], av[CPL - 1]), kWave - 1), b = read_lane(bv[CPL - 1], kWave - 1);
      h.oz = (lane == q) ? z : h.oz;
      h.ob = (lane == q) ? b : h.ob;
      if (q == kWave - 1 || j == lb) {
        if (lane <= q) *reinterpret_cast<int2 *>(hand_out + 2ull * (j - q + lane)) = make_int2(h.oz, h.ob);
        if (j != lb) strip_publish(done + strip, j);   // (the last rows are published below, after the best cell)
      }
    }
  }

  const unsigned long long err = sw.reduce_err();
  if (lane == 0 && err != ~0ull) {
    atomicMin(reinterpret_cast<unsigned long long *>(p.status + pair), err);
    atomicOr(sp.err_flag, 1u);
  }
  if constexpr (SW) {
    int score;
    unsigned long long key;
    best.reduce(col0, ncol, score, key);
    if (strip > 0 && lb > 0) merge_left_best(sp.strip_best + 4 * (slot - 1), score, key);
    const uint32_t ea = score > 0 ? (uint32_t)(key >> 32) : 0u, eb = score > 0 ? (uint32_t)key : 0u;
    if (lane == 0) {
      if (last_strip) {
        sp.score[pair] = score; sp.end_a[pair] = ea; sp.end_b[pair] = eb;
      } else {
        *reinterpret_cast<uint4 *>(sp.strip_best + 4 * slot) = make_uint4((uint32_t)score, ea, eb, 0u);
      }
    }
  } else if (last_strip) {
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      if (col0 + c + 1 == la) sp.score[pair] = sw.X[c];   // max(M, A, B) of (len_a, len_b)
  }
  if (!last_strip && lb > 0) strip_publish(done + strip, lb);   // the last rows (and the best cell so far)
}

inline uint32_t one_wave_waves(const SaScoreParams &p) { return p.f.n_pairs; }
inline uint32_t one_wave_waves(const SaScoreCrossParams &p) { return p.n_waves; }

template <int CPL, bool SW, bool CROSS, class P>
static hipError_t launch_rows_cpl(const P &p, hipStream_t stream) {
  const dim3 grid((one_wave_waves(p) + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(sa_pair_params(p).f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((score_rows_kernel<CPL, subst(), general(), SW, CROSS>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

// the columns per lane of the widest row (sa_score_row_class's steps)
template <bool SW, bool CROSS = false, class P>
static hipError_t launch_rows(const P &p, uint32_t max_len_a, hipStream_t stream) {
  const uint32_t need = columns_per_lane(max_len_a);
  return launch_by_cpl<1, 2, 3, 4, 5, 6, 8, 12, 16>(need, [&](auto cpl) { return launch_rows_cpl<cpl(), SW, CROSS>(p, stream); });
}

template <bool SW>
static hipError_t launch_strips(const SaScoreParams &p, const dim3 grid, hipStream_t stream) {
  launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((score_strips_kernel<subst(), general(), SW>), grid, dim3(kWave), table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

uint32_t sa_score_strips_per_pair(uint32_t max_len_a) {
  return max_len_a ? (uint32_t)(((uint64_t)max_len_a + sa::kScoreStripCols - 1) / sa::kScoreStripCols) : 1;
}

hipError_t sa_launch_score_rows(const SaScoreParams &p, uint32_t max_len_a, bool is_sw, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_len_a > SA_SCORE_ROW_MAX) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_ROWS, p.f.n_pairs);
  return is_sw ? sa::launch_rows<true>(p, max_len_a, stream) : sa::launch_rows<false>(p, max_len_a, stream);
}

hipError_t sa_launch_score_cross(const SaScoreCrossParams &p, uint32_t max_len_a, bool is_sw, hipStream_t stream) {
  if (p.n_waves == 0) return hipSuccess;
  if (max_len_a > SA_SCORE_ROW_MAX || p.nq == 0) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_CROSS, p.n_waves);
  return is_sw ? sa::launch_rows<true, true>(p, max_len_a, stream) : sa::launch_rows<false, true>(p, max_len_a, stream);
}

hipError_t sa_launch_score_strips(const SaScoreParams &p, bool is_sw, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_STRIPS, p.f.n_pairs);
  const dim3 grid((unsigned)blocks);
  return is_sw ? sa::launch_strips<true>(p, grid, stream) : sa::launch_strips<false>(p, grid, stream);
}
