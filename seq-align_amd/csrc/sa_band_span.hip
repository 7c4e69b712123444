// sa_band_span.hip -- banded SW hit spans (seqalign_sw_span_banded): score, start and end of the best local hit inside a band
// of diagonals, nothing stored per cell, no walk.  band_rows_kernel<.., FILL = false, SW = true>'s frame (sa_band.hip: the
// frame, its shift, the floor above the right edge, the rows swept) around SpanSweep's arithmetic (sa_span.hpp; the
// definition of a span and the tie argument: sa_span.hip's header).  The definition carries over with one
// rule more: a cell outside the band is a stop -- it holds 0 in all three states and its span is the cell itself (3.19).
//
// The kernel is sa_band_frame.hpp's band_payload_rows_kernel<BandSpanFrame, CPL, SUBST, GENERAL> -- the frame is written once, for
// this kernel and for the banded statistics kernel (sa_band_stats.hip), and the policy below says which words of SpanSweep play
// which part: one wave per pair, 4 pairs per workgroup, a frame of F = 64 x CPL positions, CPL from {1 .. 6, 8} by the launch's
// widest band.  Position g = lane * CPL + c holds column fc(j) + g on row j, fc(j) = max(1, j + d_lo).  What the
// spans do when the frame moves:
//   1. The shift.  From row 2 - d_lo on, before row j, Dx / Dy / Vx / Vy shift left by one position with X, Ap, Y, fa, arow.
//      The up-left of position 0 (boundX, boundDx / boundDy) becomes lane 0's X[0] and D[0] from before the shift: cell
//      (fc(j) - 1, j - 1), on the band's lowest diagonal.  The position that enters on the right holds 0; it lies outside the
//      band and nothing reads its spans.
//   2. Every 0 outside the band is a stop with its own coordinates.  The cell above the right edge (position g_e, column
//      j + d_hi, row j - 1) gets 0 in X, Ap, Y as in band_rows_kernel, and its vertical feed V = (j + d_hi, j - 1): only a gap
//      that pays (gap_extend > 0, or gap_open + gap_extend > 0) reads it.  The feed left of the frame is {0, 0, not from A,
//      spans (fc(j) - 1, j)} on every row, whether that cell is the border or outside the band, and SpanSweep::row makes of
//      it the up-left of position 0 on the next row, which is right while the frame stands still (the border cell (0, j)).
//      Before the first row swept, `first`, the frame stands over zeros of row first - 1: their spans are (column, first - 1).
//   3. The best cell with its span.  SpanSweep's running best per position (bs / br / bx / by), updated only for the lane's
//      ncol band columns of the row (SpanSweep::row<BAND = true>).  When the frame moves, lane 0's column retires into a
//      wave-uniform best with its span (strict >: a tie stays with the retired, lower columns) and the four arrays shift.
//      The end pick is BandBest::reduce's order: the retired best, then the live columns ascending.
//   4. Columns right of the band or of len_a: whatever the sweep computes there stays out of the best cell, out of the error
//      key (both masked by ncol) and out of the result; the gap_b scan runs left to right and never carries it into the band,
//      and before such a position's column enters the band it passes through g_e, where rule 2 resets it.
// Every loop is bounded by the rows first .. min(len_b, len_a - d_lo); there are no matrices, no hand-off and no waits but
// for the code fetches.  The launches are recorded as "band_score" (the second launch record's table is pinned).
//
// The wide form (seqalign_sw_span_banded_wide) is sa_band_frame.hpp's band_payload_strips_kernel<BandSpanFrame,
// ..> over the same policy: the rules per strip are in that header.  The two payload words are full words, so there is no limit
// on the lengths and nothing to overflow in a frame position that overhangs len_a.
#include "sa_band_frame.hpp"

namespace sa {

// the span family of the band frame (sa_band_frame.hpp): the two payload words are the stop cell's x and y
struct BandSpanFrame {
  using Params = SaBandSpanParams;
  template <int CPL, int SUBST, bool GENERAL>
  using Sweep = SpanSweep<CPL, SUBST, GENERAL>;

  // the sweep's two payload words by role: diagonal and vertical feed, the up-left of position 0, the best cell's
  template <class S>
  static __device__ __forceinline__ auto &D0(S &sw) { return sw.Dx; }
  template <class S>
  static __device__ __forceinline__ auto &D1(S &sw) { return sw.Dy; }
  template <class S>
  static __device__ __forceinline__ auto &V0(S &sw) { return sw.Vx; }
  template <class S>
  static __device__ __forceinline__ auto &V1(S &sw) { return sw.Vy; }
  template <class S>
  static __device__ __forceinline__ auto &boundD0(S &sw) { return sw.boundDx; }
  template <class S>
  static __device__ __forceinline__ auto &boundD1(S &sw) { return sw.boundDy; }
  template <class S>
  static __device__ __forceinline__ auto &best0(S &sw) { return sw.bx; }
  template <class S>
  static __device__ __forceinline__ auto &best1(S &sw) { return sw.by; }
  // start_strip has set x = the column; the zeros of row `row` are stops of their own (rule 2)
  template <class S>
  static __device__ __forceinline__ void first_row(S &sw, uint32_t, uint32_t, uint32_t row) {
    constexpr int CPL = sizeof(sw.Dy) / sizeof(sw.Dy[0]);
#pragma unroll
    for (int c = 0; c < CPL; ++c) sw.Dy[c] = sw.Vy[c] = row;
    sw.boundDy = row;
  }
  // the two words of a stop in cell (x, y): its span is the cell itself
  static __device__ __forceinline__ uint32_t stop0(uint32_t x, uint32_t y) { return x; }
  static __device__ __forceinline__ uint32_t stop1(uint32_t x, uint32_t y) { return y; }
  static __device__ __forceinline__ void write(const SaBandSpanParams &kp, uint32_t pair, int score, unsigned long long key,
                                               unsigned long long span) {
    const bool hit = score > 0;
    const uint32_t ea = hit ? (uint32_t)(key >> 32) : 0u, eb = hit ? (uint32_t)key : 0u;
    const uint32_t pa = hit ? (uint32_t)(span >> 32) : 0u, pb = hit ? (uint32_t)span : 0u;
    kp.b.score[pair] = hit ? score : 0;
    kp.pos_a[pair] = pa; kp.pos_b[pair] = pb;
    kp.len_a[pair] = ea - pa; kp.len_b[pair] = eb - pb;
  }
};

}  // namespace sa

hipError_t sa_launch_band_span(const SaBandSpanParams &p, uint32_t max_width, hipStream_t stream) {
  return sa::launch_band_payload<sa::BandSpanFrame>(p, max_width, stream);
}
hipError_t sa_launch_band_span_strips(const SaBandWideParams<SaBandSpanParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  return sa::launch_band_payload_strips<sa::BandSpanFrame>(p, strip_cols, items, stream);
}
