// sa_sw_gaps.hip -- SW gap-run counts at any length: for each pair the best local hit's score and end cell
// (seqalign_sw_score_batch's three integers) and the number of maximal runs of '-' in each of that hit's two strings, in one
// forward pass: no matrices, no traceback, no cell cap and no limit on the sequence lengths (seqalign_sw_gaps_batch).  BLAST's
// gapopen is the sum of the two.  sa_sw_counts.hip's sweep with the two run counts as the two payload words.  DESIGN.md 3.33:
//   run(cell, S)  = (0, 0) where the walk of alignment_reverse_move (tie order GAP_A, GAP_B, MATCH) that starts in state S of
//                   the cell stops in that very cell (value <= 0, a border cell, a forced gap_b, the floor candidate of its own
//                   cell), else run(the predecessor the walker picks) -- plus one in the word of S where S is a gap state,
//                   UNLESS the picked predecessor is the same gap state and is not itself a stop -- as (gap_runs_a, gap_runs_b),
//                   a word each.  The match state adds nothing.
// A run is counted at its first column in forward order, not at an "open" move: with gap_extend > 0 a gap state can extend out
// of a state whose value is 0, a stop that has emitted no column, and the run begins in the extending cell.  Counting open moves
// would miss those runs; counting every entry into a gap state would invent runs where the entered state is a stop.
// The pair follows the ONE walk sa_sw_counts.hip's two words follow, so whatever selects that pair of words selects this one: the
// D and V feeds, the one-bit merge of the gap_b scan, zwins at the seam, the running best per column.  Every feed, hand-off and
// stop is in raw form and the increment is decided where the pair is consumed (sa_sw_gaps.hpp's header), so a stop is (0, 0)
// wherever it is and the shared shells need no word of their own.  A walk has fewer than len_a + len_b < 2^31 columns, so
// neither word wraps at any length a batch can hold.
//
// The kernels are sa_payload_kernels.hpp's over SwGapsFamily below.  Rows kernel: rows of up to 512 columns, one wave per pair
// (1 .. 6 or 8 columns per lane), 4 pairs per workgroup.  Strips kernel: wider rows on the strips pipeline of sa_strips.hpp; the
// hand-off per row and strip is StripSpanHandoff's 32 bytes, the best cell so far travels as merge_left_best_span's 32 bytes
// with the two run counts where the span was.  There is no CROSS form.  Recorded as "score_rows" / "score_strips".
#include "sa_sw_gaps.hpp"
#include "sa_payload_kernels.hpp"

namespace sa {

struct SwGapsFamily {
  using Params = SaSwGapsParams;
  template <int CPL, int SUBST, bool GENERAL> using Sweep = SwGapSweep<CPL, SUBST, GENERAL>;
  static constexpr bool kBestCell = true;
  static __device__ __forceinline__ NoBorder border(const SaFillParams &) { return {}; }
  template <class S>
  static __device__ __forceinline__ void start_strip(S &sw, const SaFillParams &p, const SweepConsts &k, NoBorder,
                                                     const uint8_t *__restrict__ seq_a, uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    sw.start_strip(p, k, seq_a, la, i0, col0, lane);
  }
  // the border column: cell (0, j) holds 0, every walk stops in it with no run counted
  static __device__ __forceinline__ SpanFeed border_feed(const SweepConsts &, NoBorder, uint32_t) { return {0, 0, 0, 0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ void strip0_feed(StripSpanHandoff &h, const SweepConsts &, NoBorder, uint32_t) {
    h.in1 = make_int4(0, 0, 0, 0);   // border_feed's payloads in hand-off form
  }
  // end_a / end_b from the key, the run counts from the words (SaSwGapsParams: the span block's arrays by their new names)
  static __device__ __forceinline__ void write(const SaSwGapsParams &sp, uint64_t at, int score, unsigned long long key,
                                               unsigned long long words) {
    sw_gaps_write(sp.score, sp.pos_a, sp.pos_b, sp.len_a, sp.len_b, at, score, key, words);
  }
};

}  // namespace sa

hipError_t sa_launch_sw_gaps_rows(const SaSwGapsParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_rows<sa::SwGapsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_sw_gaps_strips(const SaSwGapsParams &p, hipStream_t stream) {
  return sa::launch_payload_strips<sa::SwGapsFamily>(p, stream);
}
