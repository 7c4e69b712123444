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
// The kernels are sa_payload_kernels.hpp's over SpanFamily below.  Rows kernel: rows of up to 512 columns, one wave per pair
// (1 .. 6 or 8 columns per lane), 4 pairs per workgroup.  Strips kernel: wider rows, the strips pipeline of sa_strips.hpp -- the
// hand-off per row and strip is 32 bytes (StripSpanHandoff: max(M, A) and B of the strip's last column, their spans, and
// whether max(M, A) came from A), the best cell so far travels with its span (merge_left_best_span).  Both are recorded as
// "score_rows" / "score_strips", the one-wave kernel's CROSS form (two sets instead of a pair list) as "score_cross".
#include "sa_span.hpp"
#include "sa_payload_kernels.hpp"

namespace sa {

struct SpanFamily {
  using Params = SaSpanParams;
  template <int CPL, int SUBST, bool GENERAL> using Sweep = SpanSweep<CPL, SUBST, GENERAL>;
  static constexpr bool kBestCell = true;
  static __device__ __forceinline__ NoBorder border(const SaFillParams &) { return {}; }
  template <class S>
  static __device__ __forceinline__ void start_strip(S &sw, const SaFillParams &p, const SweepConsts &k, NoBorder,
                                                     const uint8_t *__restrict__ seq_a, uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    sw.start_strip(p, k, seq_a, la, i0, col0, lane);
  }
  // the border column: cell (0, j) holds 0 and every walk stops in it
  static __device__ __forceinline__ SpanFeed border_feed(const SweepConsts &, NoBorder, uint32_t j) { return {0, 0, 0, 0u, j, 0u, j}; }
  static __device__ __forceinline__ void strip0_feed(StripSpanHandoff &, const SweepConsts &, NoBorder, uint32_t) {}   // as loaded
  static __device__ __forceinline__ void write(const SaSpanParams &sp, uint64_t at, int score, unsigned long long key,
                                               unsigned long long span) {
    span_write(sp, at, score, key, span);
  }
};

}  // namespace sa

uint32_t sa_span_strips_per_pair(uint32_t max_len_a) {
  return max_len_a ? (uint32_t)(((uint64_t)max_len_a + sa::kSpanStripCols - 1) / sa::kSpanStripCols) : 1;
}

hipError_t sa_launch_span_rows(const SaSpanParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_rows<sa::SpanFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_span_cross(const SaSpanCrossParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_cross<sa::SpanFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_span_strips(const SaSpanParams &p, hipStream_t stream) {
  return sa::launch_payload_strips<sa::SpanFamily>(p, stream);
}
