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
// The kernels are sa_payload_kernels.hpp's over NwStatsFamily below.  Rows kernel: rows of up to 512 columns, one wave per pair
// (1 .. 6 or 8 columns per lane), 4 pairs per workgroup, and its CROSS form (two sets instead of a pair list).  Strips kernel:
// wider rows on the strips pipeline of sa_strips.hpp; the hand-off per row and strip is StripSpanHandoff's 32 bytes with payloads
// for spans, the waits and publishes are strip_wait / strip_publish as in sa_span.hip.  There is no running best cell: the last
// strip's lane that owns column len_a holds the result after the last row.  Recorded as "score_rows" / "score_strips" /
// "score_cross".
#include "sa_nw_stats.hpp"
#include "sa_payload_kernels.hpp"

namespace sa {

struct NwStatsFamily {
  using Params = SaStatsParams;
  template <int CPL, int SUBST, bool GENERAL> using Sweep = StatSweep<CPL, SUBST, GENERAL>;
  static constexpr bool kBestCell = false;   // the result is cell (len_a, len_b)'s: StatSweep::write
  static __device__ __forceinline__ Border border(const SaFillParams &p) {
    return {p.floor, p.gap_open, p.ext, false, (p.flags & SA_F_NO_START_GAP) != 0};
  }
  template <class S>
  static __device__ __forceinline__ void start_strip(S &sw, const SaFillParams &p, const SweepConsts &k, const Border &bd,
                                                     const uint8_t *__restrict__ seq_a, uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    sw.start_strip(p, k, bd, seq_a, la, i0, col0, lane);
  }
  // the border column (reference alignment.c:72-80): gap_a holds the edge, match and gap_b the floor; every walk ends there
  static __device__ __forceinline__ StatFeed border_feed(const SweepConsts &k, const Border &bd, uint32_t j) {
    return {max(k.floor_, bd.edge_gap(j)), k.floor_, 1, 0u, 0u, 0u, 0u};
  }
  static __device__ __forceinline__ void strip0_feed(StripSpanHandoff &h, const SweepConsts &k, const Border &bd, uint32_t r) {
    h.in0 = make_int4(max(k.floor_, bd.edge_gap(r)), k.floor_, 1, 0);   // border_feed in place of SW's zeros
    h.in1 = make_int4(0, 0, 0, 0);
  }
  // cell (0, len_b) of the border column
  static __device__ __forceinline__ void write_border(const SaStatsParams &sp, const SweepConsts &k, const Border &bd, uint64_t at,
                                                      uint32_t lb) {
    sp.score[at] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
    sp.matches[at] = 0u; sp.mismatches[at] = 0u;
  }
};

}  // namespace sa

hipError_t sa_launch_stats_rows(const SaStatsParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_rows<sa::NwStatsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_stats_cross(const SaStatsCrossParams &p, uint32_t max_len_a, hipStream_t stream) {
  return sa::launch_payload_cross<sa::NwStatsFamily>(p, max_len_a, stream);
}

hipError_t sa_launch_stats_strips(const SaStatsParams &p, hipStream_t stream) {
  return sa::launch_payload_strips<sa::NwStatsFamily>(p, stream);
}
