// sa_band_counts.hip -- banded SW identity counts at any length (seqalign_sw_counts_banded, seqalign_sw_counts_banded_wide):
// score, end cell and the identity counts of the best local hit inside a band of diagonals, nothing stored per cell, no walk.
// The moving frame of sa_band_frame.hpp (the banded span kernel's, sa_band_span.hip's header: the four rules) around
// SwCountSweep's arithmetic (sa_sw_counts.hpp; the definition of the two words and the tie argument: sa_sw_counts.hip's header,
// DESIGN.md 3.32).  A cell outside the band is a stop that has counted nothing: it holds 0 in all three states and (0, 0) in both
// words.
//
// The narrow kernel is band_payload_rows_kernel<BandSwCountsFrame, CPL, SUBST, GENERAL>: one wave per pair, 4 pairs per
// workgroup, CPL from {1 .. 6, 8} by the launch's widest band.  The wide kernel is band_payload_strips_kernel<BandSwCountsFrame,
// ..>: one wave per (pair, strip of 64 | 128 | 256 | 512 columns).  What the two words do when the frame moves, rule by rule:
//   1. The shift.  Dm / Dn / Vm / Vn shift left by one position with X, Ap, Y, fa, arow; boundDm / boundDn become lane 0's
//      Dm[0] / Dn[0] from before the shift.  What enters on the right holds 0 in both words.
//   2. Zeros outside the band.  Every stop is (0, 0): the row before the first swept, the cell above the band's right edge, the
//      feed left of the frame.  start_strip has written exactly that, so first_row has nothing to set.
//   3. The best cell with both counts.  bs / br / bw0 / bw1 as in sa_band_stats.hip: lane 0's column retires into a wave-uniform
//      best with its two words, the four arrays shift, the end pick takes the retired best first, then the live columns ascending.
//   4. Columns right of the band or of len_a stay out of the best cell, out of the error key (both masked by ncol) and out of
//      the result, as in the span kernel.
//
// sa_band_stats.hip argues at length that no band cell reads the "garbage word" of a frame position right of len_a, whose
// x | y << 16 overflows its 16 bits.  That argument has no counterpart here: no word of this family holds a coordinate, a stop
// is (0, 0) at every position, and a count is bounded by min(len_a, len_b) < 2^31 in any cell, band cell or not.  What a
// position outside the band computes is still never read by a band cell (sa_band_frame.hpp's header shows that for any payload),
// but nothing would be malformed if it were looked at.
//
// Every loop is bounded as in sa_band_frame.hpp; the launches are recorded as "band_score" (the second launch record's table is
// pinned).
#include "sa_sw_counts.hpp"
#include "sa_band_frame.hpp"

namespace sa {

// the SW counts family of the band frame: word 0 matches, word 1 mismatches
struct BandSwCountsFrame {
  using Params = SaBandSwCountsParams;
  template <int CPL, int SUBST, bool GENERAL>
  using Sweep = SwCountSweep<CPL, SUBST, GENERAL>;

  // the sweep's two payload words by role: diagonal and vertical feed, the up-left of position 0, the best cell's
  template <class S>
  static __device__ __forceinline__ auto &D0(S &sw) { return sw.Dm; }
  template <class S>
  static __device__ __forceinline__ auto &D1(S &sw) { return sw.Dn; }
  template <class S>
  static __device__ __forceinline__ auto &V0(S &sw) { return sw.Vm; }
  template <class S>
  static __device__ __forceinline__ auto &V1(S &sw) { return sw.Vn; }
  template <class S>
  static __device__ __forceinline__ auto &boundD0(S &sw) { return sw.boundDm; }
  template <class S>
  static __device__ __forceinline__ auto &boundD1(S &sw) { return sw.boundDn; }
  template <class S>
  static __device__ __forceinline__ auto &best0(S &sw) { return sw.bw0; }
  template <class S>
  static __device__ __forceinline__ auto &best1(S &sw) { return sw.bw1; }
  // the zeros of row `row` have counted nothing: what start_strip wrote
  template <class S>
  static __device__ __forceinline__ void first_row(S &, uint32_t, uint32_t, uint32_t) {}
  // the two words of a stop in any cell: it has counted nothing
  static __device__ __forceinline__ uint32_t stop0(uint32_t, uint32_t) { return 0u; }
  static __device__ __forceinline__ uint32_t stop1(uint32_t, uint32_t) { return 0u; }
  // end_a / end_b from the key, the counts from the words (SaBandSwCountsParams: the span block's arrays by their new names)
  static __device__ __forceinline__ void write(const SaBandSwCountsParams &kp, uint32_t pair, int score, unsigned long long key,
                                               unsigned long long words) {
    sw_counts_write(kp.b.score, kp.pos_a, kp.pos_b, kp.len_a, kp.len_b, pair, score, key, words);
  }
};

}  // namespace sa

hipError_t sa_launch_band_sw_counts(const SaBandSwCountsParams &p, uint32_t max_width, hipStream_t stream) {
  return sa::launch_band_payload<sa::BandSwCountsFrame>(p, max_width, stream);
}
hipError_t sa_launch_band_sw_counts_strips(const SaBandWideParams<SaBandSwCountsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  return sa::launch_band_payload_strips<sa::BandSwCountsFrame>(p, strip_cols, items, stream);
}
