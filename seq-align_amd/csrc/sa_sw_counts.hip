// sa_sw_counts.hip -- SW identity counts at any length: for each pair the best local hit's score and end cell
// (seqalign_sw_score_batch's three integers) and the matches and mismatches of that hit's strings, in one forward pass: no
// matrices, no traceback, no cell cap and no limit on the sequence lengths (seqalign_sw_counts_batch).  sa_sw_stats.hip's sweep
// with the two counts as two full payload words and no stop cell.  DESIGN.md 3.32:
//   cnt(cell, S)  = (0, 0) where the walk of alignment_reverse_move (tie order GAP_A, GAP_B, MATCH) that starts in state S of
//                   the cell stops in that very cell (value <= 0, a border cell, a forced gap_b, the floor candidate of its own
//                   cell), else cnt(the predecessor the walker picks) -- plus one match or one mismatch for the cell's own
//                   letters where S is the match state -- as (matches, mismatches), a word each.
// It follows the ONE walk sa_sw_stats.hip's two words follow, so whatever selects that pair of words selects this one: the D and
// V feeds, the one-bit merge of the gap_b scan, zwins at the seam, the running best per column.  The counts do not depend on
// where the walk stops, only on which cells it passes, so dropping the stop cell changes no count; and a walk has at most
// min(len_a, len_b) letter columns, so neither word wraps at any length a batch can hold.  Start and length of the hit, where
// wanted, come from seqalign_sw_span_batch on the same batch, which has no length limit either.
//
// The kernels are sa_payload_kernels.hpp's over SwCountsFamily below.  Rows kernel: rows of up to 512 columns, one wave per pair
// (1 .. 6 or 8 columns per lane), 4 pairs per workgroup.  Strips kernel: wider rows on the strips pipeline of sa_strips.hpp; the
// hand-off per row and strip is StripSpanHandoff's 32 bytes, the best cell so far travels as merge_left_best_span's 32 bytes
// with the two counts where the span was.  There is no CROSS form.  Recorded as "score_rows" / "score_strips".
#include "sa_sw_counts.hpp"
#include "sa_payload_kernels.hpp"

namespace sa {

struct SwCountsFamily {
  using Params = SaSwCountsParams;
  template <int CPL, int SUBST, bool GENERAL> using Sweep = SwCountSweep<CPL, SUBST, GENERAL>;
  static constexpr bool kBestCell = true;
  static __device__ __forceinline__ NoBorder border(const SaFillParams &) { return {}; }
  template <class S>
  static __device__ __forceinline__ void start_strip(S &sw, const SaFillParams &p, const SweepConsts &k, NoBorder,
                                                     const uint8_t *__restrict__ seq_a, uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    sw.start_strip(p, k, seq_a, la, i0, col0, lane);
  }
  // the border column: cell (0, j) holds 0, every walk stops in it with no letters counted
  static __device__ __forceinline__ SpanFeed border_feed(const SweepConsts &, NoBorder, uint32_t) { return {0, 0, 0, 0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ void strip0_feed(StripSpanHandoff &h, const SweepConsts &, NoBorder, uint32_t) {
    h.in1 = make_int4(0, 0, 0, 0);   // border_feed's payloads in hand-off form
  }
  // end_a / end_b from the key, the counts from the words (SaSwCountsParams: the span block's arrays by their new names)
  static __device__ __forceinline__ void write(const SaSwCountsParams &sp, uint64_t at, int score, unsigned long long key,
                                               unsigned long long words) {
    sw_counts_write(sp.score, sp.pos_a, sp.pos_b, sp.len_a, sp.len_b, at, score, key, words);
  }
};

}  // namespace sa

hipError_t sa_launch_sw_counts_rows(const SaSwCountsParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_rows<sa::SwCountsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_sw_counts_strips(const SaSwCountsParams &p, hipStream_t stream) {
  return sa::launch_payload_strips<sa::SwCountsFamily>(p, stream);
}
