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
// The kernels are sa_payload_kernels.hpp's over SwStatsFamily below.  Rows kernel: rows of up to 512 columns, one wave per pair
// (1 .. 6 or 8 columns per lane), 4 pairs per workgroup, and its CROSS form (two sets instead of a pair list).  Strips kernel:
// wider rows on the strips pipeline of sa_strips.hpp; the hand-off per row and strip is StripSpanHandoff's 32 bytes, the best
// cell so far travels as merge_left_best_span's 32 bytes with the two words where the span was, the waits and publishes are
// strip_wait / strip_publish as in sa_span.hip.  Recorded as "score_rows" / "score_strips" / "score_cross".
#include "sa_sw_stats.hpp"
#include "sa_payload_kernels.hpp"

namespace sa {

struct SwStatsFamily {
  using Params = SaSwStatsParams;
  template <int CPL, int SUBST, bool GENERAL> using Sweep = SwStatSweep<CPL, SUBST, GENERAL>;
  static constexpr bool kBestCell = true;
  static __device__ __forceinline__ NoBorder border(const SaFillParams &) { return {}; }
  template <class S>
  static __device__ __forceinline__ void start_strip(S &sw, const SaFillParams &p, const SweepConsts &k, NoBorder,
                                                     const uint8_t *__restrict__ seq_a, uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    sw.start_strip(p, k, seq_a, la, i0, col0, lane);
  }
  // the border column: cell (0, j) holds 0, every walk stops in it with no letters counted
  static __device__ __forceinline__ SpanFeed border_feed(const SweepConsts &, NoBorder, uint32_t j) {
    const uint32_t here = sw_stat_cell(0, j);
    return {0, 0, 0, here, 0u, here, 0u};
  }
  static __device__ __forceinline__ void strip0_feed(StripSpanHandoff &h, const SweepConsts &, NoBorder, uint32_t r) {
    const int here = (int)sw_stat_cell(0, r);   // border_feed's packed form in place of the span's two words
    h.in1 = make_int4(here, 0, here, 0);
  }
  static __device__ __forceinline__ void write(const SaSwStatsParams &sp, uint64_t at, int score, unsigned long long key,
                                               unsigned long long words) {
    sw_stats_write(sp, at, score, key, words);
  }
};

}  // namespace sa

hipError_t sa_launch_sw_stats_rows(const SaSwStatsParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_rows<sa::SwStatsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_sw_stats_cross(const SaSwStatsCrossParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_cross<sa::SwStatsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_sw_stats_strips(const SaSwStatsParams &p, hipStream_t stream) {
  return sa::launch_payload_strips<sa::SwStatsFamily>(p, stream);
}
