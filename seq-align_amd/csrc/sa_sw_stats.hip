// sa_sw_stats.hip -- SW alignment statistics: for each pair the best local hit's score, start and end (seqalign_sw_span_batch's five
// integers) and the matches and mismatches of that hit's strings, in one forward pass: no matrices, no traceback, no cell cap
// (seqalign_sw_stats_batch / _cross).  sa_span.hip's sweep with another meaning in the two payload words carried beside each of
// a cell's states S in {match, gap_a, gap_b}.  DESIGN.md 3.22:
//   stop(cell, S) = the cell in which the walk of alignment_reverse_move (tie order GAP_A, GAP_B, MATCH) stops when it starts
//                   there: sa_span.hip's span, here packed x | y << 16;
//   cnt(cell, S)  = (0, 0) where the walk stops in that very cell (value <= 0, a border cell, a forced gap_b, the floor
//                   candidate of its own cell), else cnt(the predecessor the walker picks) -- plus one match or one mismatch
//                   for the cell's own letters where S is the match state -- packed matches | mismatches << 16.
// Both follow ONE walk, so whatever selects a span in sa_span.hip selects the pair of words here: the D and V feeds, the
// one-bit merge of the gap_b scan, zwins at the seam, the running best per column.  Unlike NW's (sa_nw_stats.hip) SW's floor is
// a stop, not a missing predecessor: no state is without a walk, there is no mark and no SEQALIGN_E_TRACEBACK.
// Why 16 bits each: both sequences have at most SA_SW_STATS_MAX_LEN = 65 535 letters (the host refuses longer ones), so x, y <=
// 65 535, and a walk has at most min(len_a, len_b) letter columns, so matches + mismatches <= 65 535 and neither half of the
// counter word carries into the other.
//
// sw_stats_rows_kernel: rows of up to 512 columns, one wave per pair (1 .. 6 or 8 columns per lane), 4 pairs per workgroup, and
// its CROSS form (two sets instead of a pair list).  sw_stats_strips_kernel: wider rows on the strips pipeline of sa_strips.hpp;
// the hand-off per row and strip is StripSpanHandoff's 32 bytes, the best cell so far travels as merge_left_best_span's 32 bytes
// with the two words where the span was, the waits and publishes are strip_wait / strip_publish as in sa_span.hip.  Recorded as
// "score_rows" / "score_strips" / "score_cross".
#include "sa_sw_stats.hpp"

namespace sa {

__device__ __forceinline__ const SaSwStatsParams &sw_stats_params(const SaSwStatsParams &p) { return p; }
__device__ __forceinline__ const SaSwStatsParams &sw_stats_params(const SaSwStatsCrossParams &p) { return p.s; }

template <int CPL, int SUBST, bool GENERAL, bool CROSS = false>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
sw_stats_rows_kernel(const std::conditional_t<CROSS, SaSwStatsCrossParams, SaSwStatsParams> kp) {
  const SaSwStatsParams &sp = sw_stats_params(kp);
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

  SwStatSweep<CPL, SUBST, GENERAL> sw;
  const uint32_t col0 = lane * CPL;
  const int ncol = max(0, min(CPL, (int)la - lane * CPL));
  sw.start_strip(p, k, sa_, la, 0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)

  int code = 0;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {   // every 64 rows: lane t fetches seq_b's code for row j + t
      const uint32_t r = j + lane;
      if (r <= lb) code = p.code[sb_[r - 1]];
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const uint32_t here = sw_stat_cell(0, j);   // the border column: cell (0, j) holds 0
    const SpanFeed f{0, 0, 0, here, 0u, here, 0u};
    SpanFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  int score;
  unsigned long long key, words;
  sw.reduce_best(col0, ncol, score, key, words);
  if (lane == 0) {
    sw_stats_write(sp, at, score, key, words);
    if constexpr (CROSS) {
      if (err != ~0ull) {
        atomicMin(kp.err_pair, (unsigned long long)at);
        atomicOr(sp.err_flag, 1u);
      }
    } else {
      p.status[pair] = err;
      if (err != ~0ull) atomicOr(sp.err_flag, 1u);
    }
  }
}

template <int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
sw_stats_strips_kernel(const SaSwStatsParams sp) {
  constexpr int CPL = kSpanStripCPL;
  const SaFillParams &p = sp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x;
  const uint32_t spp = sp.strips_per_pair;
  uint32_t strip, pair;
  strip_of_ticket(strip_ticket(sp.progress + (uint64_t)gridDim.x), spp, strip, pair);
  if (pair >= p.n_pairs) return;

  const uint32_t la = p.len_a[pair], lb = p.len_b[pair];
  const uint32_t i0 = strip * kSpanStripCols;
  if (i0 >= la && strip != 0) return;   // this pair has fewer strips
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[pair];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[pair];
  const uint32_t W = la + 1;
  const uint64_t slot = (uint64_t)pair * spp + strip;   // my progress word / strip_best entry
  uint32_t *done = sp.progress + (uint64_t)pair * spp;  // done[s] = rows strip s has handed over
  const uint64_t rows = (uint64_t)lb + 1;
  int32_t *hand_out = sp.handoff + kSpanHandoffInts * (sp.handoff_off[pair] + (uint64_t)strip * rows);
  const int32_t *hand_in = sp.handoff + kSpanHandoffInts * (sp.handoff_off[pair] + (uint64_t)(strip ? strip - 1 : 0) * rows);

  const SweepConsts k(p, table);
  const uint32_t cols = (i0 < la) ? min(kSpanStripCols, la - i0) : 0;
  const bool last_strip = i0 + kSpanStripCols >= la;
  const uint32_t col0 = i0 + lane * CPL;
  const int ncol = max(0, min(CPL, (int)cols - lane * CPL));
  SwStatSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, sa_, la, i0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);

  StripSpanHandoff h;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {
      // rows j .. j + 63 of the strip to my left must have been handed over
      if (strip > 0) strip_wait(done + strip - 1, min(j + kWave - 1, lb));
      h.load(p, sb_, lb, strip, i0, hand_in, j + lane);
      if (strip == 0) {   // the border column in packed form (see sw_stats_rows_kernel) in place of the span's two words
        const int here = (int)sw_stat_cell(0, j + lane);
        h.in1 = make_int4(here, 0, here, 0);
      }
    }
    const SpanFeed f{read_lane(h.in0.x, q), read_lane(h.in0.y, q), read_lane(h.in0.z, q),
                     (uint32_t)read_lane(h.in1.x, q), (uint32_t)read_lane(h.in1.y, q),
                     (uint32_t)read_lane(h.in1.z, q), (uint32_t)read_lane(h.in1.w, q)};
    SpanFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(h.code, q), f, out);
    if (!last_strip) {   // a strip that is not the last is full: lane 63's last column is the strip's
      const int4 o0 = make_int4(read_lane(out.z, kWave - 1), read_lane(out.b, kWave - 1), read_lane(out.from_a, kWave - 1), 0);
      const int4 o1 = make_int4(read_lane((int)out.zx, kWave - 1), read_lane((int)out.zy, kWave - 1),
                                read_lane((int)out.bx, kWave - 1), read_lane((int)out.by, kWave - 1));
      h.keep(o0, o1, hand_out, done + strip, lane, q, j, lb);
    }
  }

  const unsigned long long err = sw.reduce_err();
  if (lane == 0 && err != ~0ull) {
    atomicMin(reinterpret_cast<unsigned long long *>(p.status + pair), err);
    atomicOr(sp.err_flag, 1u);
  }
  int score;
  unsigned long long key, words;
  sw.reduce_best(col0, ncol, score, key, words);
  if (strip > 0 && lb > 0) merge_left_best_span(sp.strip_best + kSpanBestWords * (slot - 1), score, key, words);
  if (lane == 0) {
    if (last_strip) {
      sw_stats_write(sp, pair, score, key, words);
    } else {
      uint4 *entry = reinterpret_cast<uint4 *>(sp.strip_best + kSpanBestWords * slot);
      entry[0] = make_uint4((uint32_t)score, (uint32_t)(key >> 32), (uint32_t)key, 0u);
      entry[1] = make_uint4((uint32_t)(words >> 32), (uint32_t)words, 0u, 0u);
    }
  }
  if (!last_strip && lb > 0) strip_publish(done + strip, lb);   // the last rows (and the best cell so far)
}

inline uint32_t one_wave_waves(const SaSwStatsParams &p) { return p.f.n_pairs; }
inline uint32_t one_wave_waves(const SaSwStatsCrossParams &p) { return p.n_waves; }
inline const SaFillParams &fill_of(const SaSwStatsParams &p) { return p.f; }
inline const SaFillParams &fill_of(const SaSwStatsCrossParams &p) { return p.s.f; }

template <int CPL, bool CROSS, class P>
static hipError_t launch_sw_stats_rows_cpl(const P &p, hipStream_t stream) {
  const dim3 grid((one_wave_waves(p) + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(fill_of(p), [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((sw_stats_rows_kernel<CPL, subst(), general(), CROSS>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

hipError_t sa_launch_sw_stats_rows(const SaSwStatsParams &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_ROWS, p.f.n_pairs);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_len_a), [&](auto cpl) { return sa::launch_sw_stats_rows_cpl<cpl(), false>(p, stream); });
}

hipError_t sa_launch_sw_stats_cross(const SaSwStatsCrossParams &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.n_waves == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX || p.nq == 0) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_CROSS, p.n_waves);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_len_a), [&](auto cpl) { return sa::launch_sw_stats_rows_cpl<cpl(), true>(p, stream); });
}

hipError_t sa_launch_sw_stats_strips(const SaSwStatsParams &p, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_STRIPS, p.f.n_pairs);
  sa::launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((sa::sw_stats_strips_kernel<subst(), general()>), dim3((unsigned)blocks), dim3(sa::kWave),
                       table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}
