// sa_nw_gaps.hip -- NW gap-run counts: for each pair the score and the number of maximal runs of '-' in each of the two strings
// of the alignment seqalign_nw_batch returns for it, in one forward pass: no matrices, no direction bytes, no walk, any length
// (seqalign_nw_gaps_batch / _cross).  BLAST's gapopen is the sum of the two.  sa_nw_stats.hip's sweep with the two run counts as
// the two payload words.  DESIGN.md 3.34:
//   run(cell, S)  = the pair (gap_runs_a, gap_runs_b) of the walk of alignment_reverse_move (tie order GAP_A, GAP_B, MATCH) that
//                   starts in state S of the cell.  On the border, whatever the state: (0, 0) at (0, 0), (0, 1) at (x, 0) with
//                   x > 0 and (1, 0) at (0, y) with y > 0 -- the reference leaves its loop there and emits the rest as one run
//                   of gap columns.  Elsewhere run(the predecessor the walker picks) -- plus one in the word of S where S is a
//                   gap state, UNLESS the picked predecessor is the same gap state in a cell that is not on the border.  The
//                   match state adds nothing.
// The border run never merges with a run that leads to it: a walk enters (x, 0) by a match or a gap_a move and (0, y) by a match
// or a gap_b move, both of which emit a column of another kind than the border's run (gap_b columns along row 0, gap_a columns
// along column 0), and a gap state next to the border adds its own run by the rule above.  A model that puts (0, 0) on the whole
// border, as the identity counts rightly do, is wrong on every alignment that begins with a gap.
// The pair follows the ONE walk sa_nw_stats.hip's two words follow, so whatever selects that pair of words selects this one: the
// D and V feeds, the one-bit merge of the gap_b scan, zwins at the seam, the end pick.  A state the definition gives no walk
// (clamped at the floor with every candidate below it, blocked by no_mismatches, outside a band) carries the same sticky mark,
// bit 31 of word 1 (SA_STATS_NO_WALK): a string has fewer than len_a + len_b < 2^31 columns, so no count reaches it, adding one
// never clears it and there is no length limit.  The free moves of no_end_gap_penalty in the last row and column are gap
// columns and count like any other.
//
// The kernels are sa_payload_kernels.hpp's over NwGapsFamily below, the geometry of sa_nw_stats.hip's: the rows kernel (rows of
// up to 512 columns, one wave per pair, 1 .. 6 or 8 columns per lane, 4 pairs per workgroup), its CROSS form, and the strips
// kernel with StripSpanHandoff's 32 bytes per row and strip.  Recorded as "score_rows" / "score_strips" / "score_cross".
#include "sa_nw_gaps.hpp"
#include "sa_payload_kernels.hpp"

namespace sa {

struct NwGapsFamily {
  using Params = SaNwGapsParams;
  template <int CPL, int SUBST, bool GENERAL> using Sweep = NwGapSweep<CPL, SUBST, GENERAL>;
  static constexpr bool kBestCell = false;   // the result is cell (len_a, len_b)'s: NwGapSweep::write
  static __device__ __forceinline__ Border border(const SaFillParams &p) {
    return {p.floor, p.gap_open, p.ext, false, (p.flags & SA_F_NO_START_GAP) != 0};
  }
  template <class S>
  static __device__ __forceinline__ void start_strip(S &sw, const SaFillParams &p, const SweepConsts &k, const Border &bd,
                                                     const uint8_t *__restrict__ seq_a, uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    sw.start_strip(p, k, bd, seq_a, la, i0, col0, lane);
  }
  // the border column: gap_a holds the edge, match and gap_b the floor; cell (0, j), j >= 1, is one run of gap_a columns
  static __device__ __forceinline__ SpanFeed border_feed(const SweepConsts &k, const Border &bd, uint32_t j) {
    return {max(k.floor_, bd.edge_gap(j)), k.floor_, 1, 1u, 0u, 1u, 0u};
  }
  static __device__ __forceinline__ void strip0_feed(StripSpanHandoff &h, const SweepConsts &k, const Border &bd, uint32_t r) {
    h.in0 = make_int4(max(k.floor_, bd.edge_gap(r)), k.floor_, 1, 0);   // border_feed in hand-off form
    h.in1 = make_int4(1, 0, 1, 0);
  }
  // cell (0, len_b) of the border column: len_b gap_a columns, one run unless there is none
  static __device__ __forceinline__ void write_border(const SaNwGapsParams &sp, const SweepConsts &k, const Border &bd, uint64_t at,
                                                      uint32_t lb) {
    sp.score[at] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
    sp.matches[at] = lb == 0 ? 0u : 1u; sp.mismatches[at] = 0u;
  }
};

}  // namespace sa

hipError_t sa_launch_nw_gaps_rows(const SaNwGapsParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_rows<sa::NwGapsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_nw_gaps_cross(const SaNwGapsCrossParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_cross<sa::NwGapsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_nw_gaps_strips(const SaNwGapsParams &p, hipStream_t stream) {
  return sa::launch_payload_strips<sa::NwGapsFamily>(p, stream);
}
