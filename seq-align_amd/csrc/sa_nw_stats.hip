// sa_nw_stats.hip -- NW alignment statistics: for each pair the score and the matches and mismatches of the alignment
// seqalign_nw_batch returns for it, no matrices, no direction bytes, no walk, any length (seqalign_nw_stats_batch / _cross).
// sa_score.hip's NW sweep with one thing more carried beside the three values of a cell, the way sa_span.hip carries where a
// walk stops: for each of its states S in {match, gap_a, gap_b} the pair cnt(cell, S) = (matches, mismatches) of the walk of
// alignment_reverse_move (tie order GAP_A, GAP_B, MATCH; sa_trace_common.hpp) that starts there.  DESIGN.md 3.21:
//   cnt(cell, S) = (0, 0) on the border (x = 0 or y = 0: the reference leaves its loop there and only emits gap columns),
//                  else cnt(pred) -- plus one match or one mismatch for the cell's own letters where S is the match state --
//                  pred = the first of GAP_A, GAP_B, MATCH at the predecessor cell that the walker's predicate admits and
//                  whose value plus the step's penalty equals the state's value.
// Every state value is max(candidates, floor): the equality holds for some candidate exactly when the largest one is not below
// the floor, and then for the argmax in that priority.  (A state the predicates exclude holds the floor, so it never exceeds the
// match state beside it: skipping it is all the predicates ask.)  A state clamped to the floor with every candidate below it,
// and the match state of a cell no_mismatches blocks, have no predecessor: they carry a sticky mark, bit 31 of the mismatch
// word (SA_STATS_NO_WALK; counts stay below 2^31 and adding 1 never clears it).  The result is cnt of the state the reference's
// end pick takes at (len_a, len_b) -- gap_a if it holds the maximum, else gap_b, else match -- and SEQALIGN_E_TRACEBACK where
// that state carries the mark.
//
// What crosses a row, per column: two merged payloads of the previous row's cell, both chosen when that row ends --
//   D  the diagonal feed of M(x+1, y+1): cnt of the first of A, B, M (admitted) that holds the maximum.  It is also the end
//      pick's payload in the corner cell, and gap_a's in the last column under no_end_gap_penalty (no penalty: the same pick);
//   V  the vertical feed of A(x, y+1):   A + ext first, then B, then M, each + open1.
// Whether the state that takes a feed has a walk at all is known only where it is computed (its largest candidate against the
// floor), so the mark is set there.
// Within a row gap_b's payload rides the (max,+) scan as a span does (sa_span.hip): a candidate only ever meets one that lies to
// its right, and that one wins a tie exactly when it is an opening from an admitted gap_a -- the walker, going left, takes such
// an opening as soon as it meets one, walks on while the chain continues, and takes an opening from match only when nothing
// lies further left.  Unlike SW's 0 the NW floor is no source: a cell whose candidates all lie below it is clamped, its payload
// is the mark, and it loses a tie to every candidate (strict > where it enters, nm = 0 afterwards).  So SpanCand's merge,
// L.v >= R.v + R.nm ? L : R, carries over unchanged; tests/test_nw_stats_argument_cpu.py checks every gap_b cell against the
// step-by-step walk.
//
// stats_rows_kernel: rows of up to 512 columns, one wave per pair (1 .. 6 or 8 columns per lane), 4 pairs per workgroup, and its
// CROSS form (two sets instead of a pair list).  stats_strips_kernel: wider rows on the strips pipeline of sa_strips.hpp; the
// hand-off per row and strip is StripSpanHandoff's 32 bytes with payloads for spans, the waits and publishes are strip_wait /
// strip_publish as in sa_span.hip.  There is no running best cell: the last strip's lane that owns column len_a holds the
// result after the last row.  Recorded as "score_rows" / "score_strips" / "score_cross".
#include "sa_nw_stats.hpp"

namespace sa {

__device__ __forceinline__ const SaStatsParams &stats_params(const SaStatsParams &p) { return p; }
__device__ __forceinline__ const SaStatsParams &stats_params(const SaStatsCrossParams &p) { return p.s; }

template <int CPL, int SUBST, bool GENERAL, bool CROSS = false>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
stats_rows_kernel(const std::conditional_t<CROSS, SaStatsCrossParams, SaStatsParams> kp) {
  const SaStatsParams &sp = stats_params(kp);
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
  const Border bd{p.floor, p.gap_open, p.ext, false, (p.flags & SA_F_NO_START_GAP) != 0};

  StatSweep<CPL, SUBST, GENERAL> sw;
  const uint32_t col0 = lane * CPL;
  const int ncol = max(0, min(CPL, (int)la - lane * CPL));
  sw.start_strip(p, k, bd, sa_, la, 0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)

  int code = 0;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {   // every 64 rows: lane t fetches seq_b's code for row j + t
      const uint32_t r = j + lane;
      if (r <= lb) code = p.code[sb_[r - 1]];
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    // the border column (reference alignment.c:72-80): gap_a holds the edge, match and gap_b the floor; every walk ends there
    const StatFeed f{max(k.floor_, bd.edge_gap(j)), k.floor_, 1, 0u, 0u, 0u, 0u};
    StatFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  if (la == 0) {   // cell (0, len_b) of the border column
    if (lane == 0) {
      sp.score[at] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
      sp.matches[at] = 0u; sp.mismatches[at] = 0u;
    }
  } else {
    sw.write(sp, at, col0, la);
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

template <int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
stats_strips_kernel(const SaStatsParams sp) {
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
  uint32_t *done = sp.progress + (uint64_t)pair * spp;  // done[s] = rows strip s has handed over
  const uint64_t rows = (uint64_t)lb + 1;
  int32_t *hand_out = sp.handoff + kSpanHandoffInts * (sp.handoff_off[pair] + (uint64_t)strip * rows);
  const int32_t *hand_in = sp.handoff + kSpanHandoffInts * (sp.handoff_off[pair] + (uint64_t)(strip ? strip - 1 : 0) * rows);

  const SweepConsts k(p, table);
  const Border bd{p.floor, p.gap_open, p.ext, false, (p.flags & SA_F_NO_START_GAP) != 0};
  const uint32_t cols = (i0 < la) ? min(kSpanStripCols, la - i0) : 0;
  const bool last_strip = i0 + kSpanStripCols >= la;
  const uint32_t col0 = i0 + lane * CPL;
  const int ncol = max(0, min(CPL, (int)cols - lane * CPL));
  StatSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, bd, sa_, la, i0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);

  StripSpanHandoff h;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {
      // rows j .. j + 63 of the strip to my left must have been handed over
      if (strip > 0) strip_wait(done + strip - 1, min(j + kWave - 1, lb));
      h.load(p, sb_, lb, strip, i0, hand_in, j + lane);
      if (strip == 0) {   // the NW border column in place of SW's zeros (see stats_rows_kernel)
        h.in0 = make_int4(max(k.floor_, bd.edge_gap(j + lane)), k.floor_, 1, 0);
        h.in1 = make_int4(0, 0, 0, 0);
      }
    }
    const StatFeed f{read_lane(h.in0.x, q), read_lane(h.in0.y, q), read_lane(h.in0.z, q),
                     (uint32_t)read_lane(h.in1.x, q), (uint32_t)read_lane(h.in1.y, q),
                     (uint32_t)read_lane(h.in1.z, q), (uint32_t)read_lane(h.in1.w, q)};
    StatFeed out;
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
  if (last_strip) sw.write(sp, pair, col0, la);
  else if (lb > 0) strip_publish(done + strip, lb);   // the last rows
}

inline uint32_t one_wave_waves(const SaStatsParams &p) { return p.f.n_pairs; }
inline uint32_t one_wave_waves(const SaStatsCrossParams &p) { return p.n_waves; }
inline const SaFillParams &fill_of(const SaStatsParams &p) { return p.f; }
inline const SaFillParams &fill_of(const SaStatsCrossParams &p) { return p.s.f; }

template <int CPL, bool CROSS, class P>
static hipError_t launch_stats_rows_cpl(const P &p, hipStream_t stream) {
  const dim3 grid((one_wave_waves(p) + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(fill_of(p), [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((stats_rows_kernel<CPL, subst(), general(), CROSS>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

hipError_t sa_launch_stats_rows(const SaStatsParams &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_ROWS, p.f.n_pairs);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_len_a), [&](auto cpl) { return sa::launch_stats_rows_cpl<cpl(), false>(p, stream); });
}

hipError_t sa_launch_stats_cross(const SaStatsCrossParams &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.n_waves == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX || p.nq == 0) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_CROSS, p.n_waves);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_len_a), [&](auto cpl) { return sa::launch_stats_rows_cpl<cpl(), true>(p, stream); });
}

hipError_t sa_launch_stats_strips(const SaStatsParams &p, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_STRIPS, p.f.n_pairs);
  sa::launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((sa::stats_strips_kernel<subst(), general()>), dim3((unsigned)blocks), dim3(sa::kWave),
                       table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}
