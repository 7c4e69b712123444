// sa_span.hip -- SW hit spans: the best local hit's score, start and end of each pair, no matrices, no traceback, any length
// (seqalign_sw_span_batch).  sa_score.hip's SW sweep with one thing more carried beside the three values of a cell: for each
// of its states S in {match, gap_a, gap_b} the SPAN of (cell, S) -- the cell in which the reference's walk
// (alignment_reverse_move, tie order GAP_A, GAP_B, MATCH; sa_trace_common.hpp) stops when it starts there.  DESIGN.md 3.18:
//   span(cell, S) = the cell itself where value(cell, S) <= 0 or the cell is on the border,
//                   else span(predecessor the walker picks).
// The walker's no_gaps_in_a / _b predicates never change a span: a state they exclude holds the floor 0, and where a 0 still
// ties for the maximum every state of that predecessor holds 0, so each of them stops in that very cell.
//
// What crosses a row, per column: two merged spans of the previous row's cell, both chosen when that row ends --
//   D  the diagonal feed of M(x+1, y+1): the span of the argmax of A, B, M, priority A > B > M;
//   V  the vertical feed of A(x, y+1):   A + ext first, then B, then M, each + open1.
// Within a row gap_b's span rides the (max,+) scan: the scan's element is {value, span, one bit}, its operator the maximum
// by (value, tie key).  A candidate for B(g) enters the chain at a column k <= g; the walker, going left from g, takes an
// opening from A as soon as it meets one, walks on while the chain continues, stops in a gap_b cell that holds 0 (possible
// only with gap_extend > 0: the floor is a source), and takes an opening from M only when nothing lies further left.  As a
// total order on candidates of equal value (tests/test_sw_span_argument_cpu.py checks it against the step-by-step walk):
//   opening from M at k: -k - 2   (the earliest wins, below everything else)
//   the chain coming in from the strip to the left: -1
//   opening from A at k: 2k       (the latest wins)
//   the floor at k: 2k + 1        (beats what lies at or left of it, loses to a later opening from A)
// The kernel never forms the key.  It only ever merges a candidate (or a run of them) L with one that lies to its RIGHT, R,
// and between such two the order says: R wins a tie unless R is an opening from M.  So a candidate carries one bit, nm = "not
// an opening from M", and the merge is  L.v >= R.v + R.nm ? L : R  -- one add and one compare.
//
// span_rows_kernel: rows of up to 512 columns, one wave per pair (1 .. 6 or 8 columns per lane), 4 pairs per workgroup.
// span_strips_kernel: wider rows, the strips pipeline of sa_strips.hpp -- the hand-off per row and strip is 32 bytes
// (StripSpanHandoff: max(M, A) and B of the strip's last column, their spans, and whether max(M, A) came from A), the best
// cell so far travels with its span (merge_left_best_span).  Both are recorded as "score_rows" / "score_strips", the
// one-wave kernel's CROSS form (two sets instead of a pair list) as "score_cross".
#include "sa_span.hpp"

namespace sa {

__device__ __forceinline__ const SaSpanParams &span_params(const SaSpanParams &p) { return p; }
__device__ __forceinline__ const SaSpanParams &span_params(const SaSpanCrossParams &p) { return p.s; }

// CROSS (seqalign_sw_span_cross, kind "score_cross"): sa_score.hip's CROSS form of this kernel -- wave w of a launch for one
// row class takes target t_order[w / nq] and query q_list[w % nq], longest targets first, writes its five words at
// [q * n_t + t] of the tile and leaves a failing pair's tile-local index in one 64-bit atomicMin.  Same sweep, same picks.
template <int CPL, int SUBST, bool GENERAL, bool CROSS = false>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
span_rows_kernel(const std::conditional_t<CROSS, SaSpanCrossParams, SaSpanParams> kp) {
  const SaSpanParams &sp = span_params(kp);
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

  SpanSweep<CPL, SUBST, GENERAL> sw;
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
    const SpanFeed f{0, 0, 0, 0u, j, 0u, j};   // the border column: cell (0, j) holds 0
    SpanFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  int score;
  unsigned long long key, span;
  sw.reduce_best(col0, ncol, score, key, span);
  if (lane == 0) {
    span_write(sp, at, score, key, span);
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
span_strips_kernel(const SaSpanParams sp) {
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
  SpanSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, sa_, la, i0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);

  StripSpanHandoff h;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {
      // rows j .. j + 63 of the strip to my left must have been handed over
      if (strip > 0) strip_wait(done + strip - 1, min(j + kWave - 1, lb));
      h.load(p, sb_, lb, strip, i0, hand_in, j + lane);
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
  unsigned long long key, span;
  sw.reduce_best(col0, ncol, score, key, span);
  if (strip > 0 && lb > 0) merge_left_best_span(sp.strip_best + kSpanBestWords * (slot - 1), score, key, span);
  if (lane == 0) {
    if (last_strip) {
      span_write(sp, pair, score, key, span);
    } else {
      uint4 *entry = reinterpret_cast<uint4 *>(sp.strip_best + kSpanBestWords * slot);
      entry[0] = make_uint4((uint32_t)score, (uint32_t)(key >> 32), (uint32_t)key, 0u);
      entry[1] = make_uint4((uint32_t)(span >> 32), (uint32_t)span, 0u, 0u);
    }
  }
  if (!last_strip && lb > 0) strip_publish(done + strip, lb);   // the last rows (and the best cell so far)
}

inline uint32_t one_wave_waves(const SaSpanParams &p) { return p.f.n_pairs; }
inline uint32_t one_wave_waves(const SaSpanCrossParams &p) { return p.n_waves; }
inline const SaFillParams &fill_of(const SaSpanParams &p) { return p.f; }
inline const SaFillParams &fill_of(const SaSpanCrossParams &p) { return p.s.f; }

template <int CPL, bool CROSS, class P>
static hipError_t launch_span_rows_cpl(const P &p, hipStream_t stream) {
  const dim3 grid((one_wave_waves(p) + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(fill_of(p), [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((span_rows_kernel<CPL, subst(), general(), CROSS>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

uint32_t sa_span_strips_per_pair(uint32_t max_len_a) {
  return max_len_a ? (uint32_t)(((uint64_t)max_len_a + sa::kSpanStripCols - 1) / sa::kSpanStripCols) : 1;
}

hipError_t sa_launch_span_rows(const SaSpanParams &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_ROWS, p.f.n_pairs);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_len_a), [&](auto cpl) { return sa::launch_span_rows_cpl<cpl(), false>(p, stream); });
}

hipError_t sa_launch_span_cross(const SaSpanCrossParams &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.n_waves == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX || p.nq == 0) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_CROSS, p.n_waves);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_len_a), [&](auto cpl) { return sa::launch_span_rows_cpl<cpl(), true>(p, stream); });
}

hipError_t sa_launch_span_strips(const SaSpanParams &p, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_STRIPS, p.f.n_pairs);
  sa::launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((sa::span_strips_kernel<subst(), general()>), dim3((unsigned)blocks), dim3(sa::kWave),
                       table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}
