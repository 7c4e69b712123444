// sa_band_stats.hip -- banded SW statistics (seqalign_sw_stats_banded): score, start, end and the identity counts of the best
// local hit inside a band of diagonals, nothing stored per cell, no walk.  The moving frame of sa_band_frame.hpp (the banded span
// kernel's, sa_band_span.hip's header: the four rules) around SwStatSweep's arithmetic (sa_sw_stats.hpp; the definition of the
// two packed words and the tie argument: sa_sw_stats.hip's header).  A cell outside the band is a stop that has
// counted nothing: it holds 0 in all three states, word 0 is the cell itself and word 1 is 0.
//
// The kernel (band_sw_stats_rows_kernel in DESIGN.md 3.24) is band_payload_rows_kernel<BandSwStatsFrame, CPL, SUBST, GENERAL>: one
// wave per pair, 4 pairs per workgroup, CPL from {1 .. 6, 8} by the launch's widest band, the policy below.  What
// the two words do when the frame moves, rule by rule:
//   1. The shift.  Ds / Dc / Vs / Vc shift left by one position with X, Ap, Y, fa, arow; boundDs / boundDc become lane 0's
//      Ds[0] / Dc[0] from before the shift: cell (fc(j) - 1, j - 1) on the band's lowest diagonal.  What enters on the right
//      holds 0 in both words; it lies outside the band and nothing reads it.
//   2. Zeros outside the band.  Before the first row swept, `first`, Ds = Vs = sw_stat_cell(column, first - 1), Dc = Vc = 0.  The
//      cell above the right edge (position g_e, column j + d_hi, row j - 1) gets 0 in X, Ap, Y, Vs = sw_stat_cell(j + d_hi,
//      j - 1) and Vc = 0: only a gap that pays reads it, and that gap has counted nothing.  The feed left of the frame is {0, 0,
//      not from A, cell (fc(j) - 1, j), counts 0} in both payloads.
//   3. The best cell with both words.  bs / br / bw0 / bw1 are updated only for the lane's ncol band columns of the row
//      (SwStatSweep::row<BAND = true>).  When the frame moves, lane 0's column retires into a wave-uniform best with its two
//      words (strict >: a tie stays with the retired, lower columns) and the four arrays shift.  The end pick takes the retired
//      best first, then the live columns ascending.
//   4. Columns right of the band or of len_a stay out of the best cell, out of the error key (both masked by ncol) and out of
//      the result, as in the span kernel.
//
// Rule 4 under 16-bit coordinates.  Word 0 is x | y << 16, which is right only while x <= 65 535.  The host admits len_a, len_b
// <= 65 535, so every band cell (x, j) has 1 <= x <= len_a and 1 <= j <= len_b and its own word `gx | j << 16` is exact.  A frame
// position right of len_a or right of the band can compute gx = fc(j) + g up to len_a + F - 1 > 65 535, and then its word 0 is
// garbage: x's high bits land in y.  No band cell ever reads such a word, because a band cell (x, j) reads exactly
//   - its up-left (x - 1, j - 1), on its own diagonal: a band cell, a border cell (row 0 through first_row, column 0 through the
//     feed and boundDs) or, on the lowest diagonal after a shift, lane 0's Ds[0] from before the shift, which was a band cell;
//   - the cell above it (x, j - 1), on diagonal x - j + 1 <= d_hi + 1: a band cell, or position g_e, which rule 2 has just
//     overwritten with sw_stat_cell(j + d_hi, j - 1) -- and x = j + d_hi <= len_a there, since (x, j) is a band cell;
//   - along the row, what the gap_b scan carries: the scan runs left to right (wave_scan_span takes from lower lanes only, the
//     per-lane chain from lower c only), the band columns of a row are the frame's FIRST n_row positions, and position 0 is fed
//     by the feed cell (fc(j) - 1, j) with fc(j) - 1 <= len_a; so a band cell sees band cells and the feed, never a position to
//     its right.
// A position whose column is right of the band on row j enters the band, if ever, on a later row by passing through g_e first
// (the band's right edge moves one column per row, and so does the frame from row 2 - d_lo on; before that the edge walks over
// the positions one at a time), where rule 2 resets everything a band cell reads of it: X, Ap, Y, Vs, Vc.  Its Ds / Dc are read
// only by the cell below-right of it, which lies one diagonal further right and is no band cell either.  The zeros of row
// first - 1 are written with the column in the low half too; those right of len_a or of column first - 1 + d_hi + 1 are garbage
// of the same kind and are covered by the same argument (the first row's g_e is column first + d_hi).  Columns right of len_a
// never enter the band at all.  So no mask is needed, and none is applied; tests/test_gpu_sw_stats_banded.py runs both
// sequences at 65 535 letters with the frame overhanging len_a to catch a mistake in this.
// Word 1 needs no argument: matches + mismatches <= min(len_a, len_b) <= 65 535 in any cell, band or not.
//
// Every loop is bounded by the rows first .. min(len_b, len_a - d_lo); no matrices, no hand-off, no waits but for the code
// fetches.  The launches are recorded as "band_score" (the second launch record's table is pinned).
//
// The wide form (seqalign_sw_stats_banded_wide) is sa_band_frame.hpp's band_payload_strips_kernel<
// BandSwStatsFrame, ..> over the same policy.  The 16-bit argument, per strip: a frame position right of len_a or right of the
// strip's end c0 + S can compute gx = fc(j) + g up to len_a + S - 1 > 65 535, and its word 0 is then garbage.  That header shows
// cell by cell that a band cell of a strip reads only band cells (whose own word `x | j << 16` is exact, 1 <= x <= len_a), stops
// in columns <= len_a and hand-off entries of band cells of the left strip, never such a position; so no mask is needed there
// either, and tests/test_gpu_sw_stats_banded_wide.py runs both sequences at 65 535 letters over 1 024 strips with the last
// frames overhanging len_a to catch a mistake in this.  Word 1 needs no argument, as above.
#include "sa_sw_stats.hpp"
#include "sa_band_frame.hpp"

namespace sa {

// the SW statistics family of the band frame: word 0 the stop cell x | y << 16, word 1 matches | mismatches << 16
struct BandSwStatsFrame {
  using Params = SaBandSwStatsParams;
  template <int CPL, int SUBST, bool GENERAL>
  using Sweep = SwStatSweep<CPL, SUBST, GENERAL>;

  // the sweep's two payload words by role: diagonal and vertical feed, the up-left of position 0, the best cell's
  template <class S>
  static __device__ __forceinline__ auto &D0(S &sw) { return sw.Ds; }
  template <class S>
  static __device__ __forceinline__ auto &D1(S &sw) { return sw.Dc; }
  template <class S>
  static __device__ __forceinline__ auto &V0(S &sw) { return sw.Vs; }
  template <class S>
  static __device__ __forceinline__ auto &V1(S &sw) { return sw.Vc; }
  template <class S>
  static __device__ __forceinline__ auto &boundD0(S &sw) { return sw.boundDs; }
  template <class S>
  static __device__ __forceinline__ auto &boundD1(S &sw) { return sw.boundDc; }
  template <class S>
  static __device__ __forceinline__ auto &best0(S &sw) { return sw.bw0; }
  template <class S>
  static __device__ __forceinline__ auto &best1(S &sw) { return sw.bw1; }
  // the zeros of row `row` are stops of their own that have counted nothing (start_strip has zeroed the counts)
  template <class S>
  static __device__ __forceinline__ void first_row(S &sw, uint32_t i0, uint32_t col0, uint32_t row) {
    constexpr int CPL = sizeof(sw.Ds) / sizeof(sw.Ds[0]);
#pragma unroll
    for (int c = 0; c < CPL; ++c) sw.Ds[c] = sw.Vs[c] = sw_stat_cell(col0 + c + 1, row);
    sw.boundDs = sw_stat_cell(i0, row);
  }
  // the two words of a stop in cell (x, y): the cell itself, and it has counted nothing
  static __device__ __forceinline__ uint32_t stop0(uint32_t x, uint32_t y) { return sw_stat_cell(x, y); }
  static __device__ __forceinline__ uint32_t stop1(uint32_t x, uint32_t y) { return 0u; }
  // sw_stats_write's unpacking into the banded record
  static __device__ __forceinline__ void write(const SaBandSwStatsParams &kp, uint32_t pair, int score, unsigned long long key,
                                               unsigned long long words) {
    const bool hit = score > 0;
    const uint32_t ea = hit ? (uint32_t)(key >> 32) : 0u, eb = hit ? (uint32_t)key : 0u;
    const uint32_t w0 = hit ? (uint32_t)(words >> 32) : 0u, w1 = hit ? (uint32_t)words : 0u;
    const uint32_t pa = w0 & 0xffffu, pb = w0 >> 16;
    kp.b.score[pair] = hit ? score : 0;
    kp.pos_a[pair] = pa; kp.pos_b[pair] = pb;
    kp.len_a[pair] = ea - pa; kp.len_b[pair] = eb - pb;
    kp.matches[pair] = w1 & 0xffffu; kp.mismatches[pair] = w1 >> 16;
  }
};

}  // namespace sa

hipError_t sa_launch_band_sw_stats(const SaBandSwStatsParams &p, uint32_t max_width, hipStream_t stream) {
  return sa::launch_band_payload<sa::BandSwStatsFrame>(p, max_width, stream);
}
hipError_t sa_launch_band_sw_stats_strips(const SaBandWideParams<SaBandSwStatsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  return sa::launch_band_payload_strips<sa::BandSwStatsFrame>(p, strip_cols, items, stream);
}
