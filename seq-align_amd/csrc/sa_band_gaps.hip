// sa_band_gaps.hip -- banded SW gap-run counts at any length (seqalign_sw_gaps_banded, seqalign_sw_gaps_banded_wide): score,
// end cell and the numbers of '-' runs in the two strings of the best local hit inside a band of diagonals, nothing stored per
// cell, no walk.  The moving frame of sa_band_frame.hpp (the banded span kernel's, sa_band_span.hip's header: the four rules)
// around SwGapSweep's arithmetic (sa_sw_gaps.hpp; the definition of the two words and the tie argument: sa_sw_gaps.hip's header,
// DESIGN.md 3.33).  A cell outside the band is a stop that has emitted no column: it holds 0 in all three states and (0, 0) in
// both words, and a gap state that extends out of it begins its run in the extending cell -- the sweep decides that from the
// VALUE it reads (the gap_a above <= 0, the left feed's B <= 0), which rule 2 below sets to 0, so the frame needs no word for it.
//
// The narrow kernel is band_payload_rows_kernel<BandSwGapsFrame, CPL, SUBST, GENERAL>: one wave per pair, 4 pairs per
// workgroup, CPL from {1 .. 6, 8} by the launch's widest band.  The wide kernel is band_payload_strips_kernel<BandSwGapsFrame,
// ..>: one wave per (pair, strip of 64 | 128 | 256 | 512 columns).  What the two words do when the frame moves, rule by rule:
//   1. The shift.  Da / Db / Va / Vb shift left by one position with X, Ap, Y, fa, arow; boundDa / boundDb become lane 0's
//      Da[0] / Db[0] from before the shift.  What enters on the right holds 0 in both words.
//   2. Zeros outside the band.  Every stop is (0, 0): the row before the first swept, the cell above the band's right edge
//      (whose Ap the shell resets to 0 with its V words), the feed left of the frame (B = 0).  start_strip has written exactly
//      that, so first_row has nothing to set.
//   3. The best cell with both run counts.  bs / br / bw0 / bw1 as in sa_band_counts.hip: lane 0's column retires into a
//      wave-uniform best with its two words, the four arrays shift, the end pick takes the retired best first, then the live
//      columns ascending.
//   4. Columns right of the band or of len_a stay out of the best cell, out of the error key (both masked by ncol) and out of
//      the result, as in the span kernel.
// No word of this family holds a coordinate: a stop is (0, 0) at every position and a count is below len_a + len_b < 2^31 in
// any cell, band cell or not.  What a position outside the band computes is never read by a band cell (sa_band_frame.hpp's
// header shows that for any payload).
//
// Every loop is bounded as in sa_band_frame.hpp; the launches are recorded as "band_score" (the second launch record's table is
// pinned).
#include "sa_sw_gaps.hpp"
#include "sa_band_frame.hpp"

namespace sa {

// the SW gap-run family of the band frame: word 0 gap_runs_a, word 1 gap_runs_b
struct BandSwGapsFrame {
  using Params = SaBandSwGapsParams;
  template <int CPL, int SUBST, bool GENERAL>
  using Sweep = SwGapSweep<CPL, SUBST, GENERAL>;

  // the sweep's two payload words by role: diagonal and vertical feed, the up-left of position 0, the best cell's
  template <class S>
  static __device__ __forceinline__ auto &D0(S &sw) { return sw.Da; }
  template <class S>
  static __device__ __forceinline__ auto &D1(S &sw) { return sw.Db; }
  template <class S>
  static __device__ __forceinline__ auto &V0(S &sw) { return sw.Va; }
  template <class S>
  static __device__ __forceinline__ auto &V1(S &sw) { return sw.Vb; }
  template <class S>
  static __device__ __forceinline__ auto &boundD0(S &sw) { return sw.boundDa; }
  template <class S>
  static __device__ __forceinline__ auto &boundD1(S &sw) { return sw.boundDb; }
  template <class S>
  static __device__ __forceinline__ auto &best0(S &sw) { return sw.bw0; }
  template <class S>
  static __device__ __forceinline__ auto &best1(S &sw) { return sw.bw1; }
  // the zeros of row `row` have emitted no column: what start_strip wrote
  template <class S>
  static __device__ __forceinline__ void first_row(S &, uint32_t, uint32_t, uint32_t) {}
  // the two words of a stop in any cell: it has emitted no column
  static __device__ __forceinline__ uint32_t stop0(uint32_t, uint32_t) { return 0u; }
  static __device__ __forceinline__ uint32_t stop1(uint32_t, uint32_t) { return 0u; }
  // end_a / end_b from the key, the run counts from the words (SaBandSwGapsParams: the span block's arrays by their new names)
  static __device__ __forceinline__ void write(const SaBandSwGapsParams &kp, uint32_t pair, int score, unsigned long long key,
                                               unsigned long long words) {
    sw_gaps_write(kp.b.score, kp.pos_a, kp.pos_b, kp.len_a, kp.len_b, pair, score, key, words);
  }
};

}  // namespace sa

hipError_t sa_launch_band_sw_gaps(const SaBandSwGapsParams &p, uint32_t max_width, hipStream_t stream) {
  return sa::launch_band_payload<sa::BandSwGapsFrame>(p, max_width, stream);
}
hipError_t sa_launch_band_sw_gaps_strips(const SaBandWideParams<SaBandSwGapsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  return sa::launch_band_payload_strips<sa::BandSwGapsFrame>(p, strip_cols, items, stream);
}
