// sa_band_nw_stats.hip -- banded NW statistics (seqalign_nw_stats_banded): for each pair the banded end value of
// seqalign_nw_score_banded and the matches and mismatches of the alignment inside the band that ends there, nothing stored per
// cell, no walk.  StatSweep's row arithmetic (sa_nw_stats.hpp; the definition of the payloads, the mark and the tie rule:
// sa_nw_stats.hip's header) inside the NW frame of band_rows_kernel<.., SW = false> (sa_band.hip's header: the
// frame, the three phases of the feed, why the band's edges are exact).  DESIGN.md 3.25.
//
// band_nw_stats_rows_kernel<CPL, SUBST, GENERAL>: one wave per pair, 4 pairs per workgroup, a frame of F = 64 x CPL positions,
// CPL from {1 .. 6, 8} by the launch's widest band.  Position g = lane * CPL + c holds column fc(j) + g on row j, fc(j) =
// max(1, j + d_lo), d_lo <= 0 <= d_hi.  A sibling of band_payload_rows_kernel (sa_band_frame.hpp, the SW payload frame) that
// shares frame_shift (sa_band_pipe.hpp) with it and nothing else; what differs from the SW frame:
//   No best cell, no retire.  Both corners are in every NW band, so every row 1 .. len_b is swept and the result is the last
//   row's position len_a - fc(len_b): its X and its diagonal feed Dm / Dn, the end pick's payload as in StatSweep::write.
//   A cell outside the band is no stop.  It holds the floor in all three states, and a state at the floor with no candidate has
//   no walk: its payload is the sticky mark (0, SA_STATS_NO_WALK), never the border's (0, 0).  A band cell whose best candidate
//   is such a cell either stays below the floor itself (then StatSweep::row marks it) or carries the mark on from the feed.
// The four rules of payloads in a moving frame (sa_band_span.hip's header), as they read here:
//   1. The shift.  From row -d_lo + 2 on the frame moves one column per row: Dm / Dn / Vm / Vn shift left by one position with
//      X, Ap, Y, fa, arow, and boundX / boundDm / boundDn become lane 0's X[0] / Dm[0] / Dn[0] from before the shift: cell
//      (fc(j) - 1, j - 1), on the band's lowest diagonal.  What enters on the right is column fc(j) + F - 1 of row j - 1, on
//      diagonal d_lo + F > d_hi: outside the band, the floor and the mark.
//   2. The floor outside the band.  The feed left of the frame has three phases.  Rows j <= -d_lo: the border column is in the
//      band and the feed is the unbanded kernel's border feed (NwStatsFamily::border_feed: gap_a holds the edge, counts (0, 0),
//      no mark).  Row -d_lo + 1: the feed cell (0, j) is outside the band -- the floor and the mark in both of its payloads --
//      and the frame does not move yet; the up-left of position 0 is still the border cell (0, -d_lo), which StatSweep::row
//      kept from the previous row's feed (or cell (0, 0) from start_strip when d_lo = 0).  From row -d_lo + 2 on: the same feed,
//      and rule 1 overwrites what row() derived from it for the up-left.
//      The cell above the right edge -- position g_e = j + d_hi - fc(j), column j + d_hi of row j - 1 -- is read two ways by the
//      band cell below it: through V (gap_a: Y, Ap, Vm, Vn), and, under no_end_gap_penalty in the last column, through D
//      (a_free takes max(Y, Ap) and Dm[c] / Dn[c] of its own position).  So before row j position g_e gets the floor in X, Ap, Y
//      and the mark in Vm / Vn AND in Dm / Dn.  Resetting D there harms no band cell: D of position g_e is read by that a_free
//      cell, which must see the mark, and otherwise only as the up-left of the cell below-right of it, (j + d_hi + 1, j), on
//      diagonal d_hi + 1: one diagonal outside the band.
//      Row 0 is StatSweep::start_strip's border: columns 1 .. d_hi are band cells (the edge gap, counts (0, 0)); column
//      d_hi + 1 is position g_e of row 1 and is reset there; the columns beyond it keep the edge gap until the edge walks over
//      them (below), which is as good as holding the floor from the start, since nothing reads them before.
//   3. (The best cell: none.)
//   4. Positions without a band cell -- right of the band on this row, or right of len_a -- compute whatever they compute; ncol
//      keeps them out of the error key and nothing is stored from them.  No band cell reads one.  A band cell (x, j) reads
//        - its up-left (x - 1, j - 1), on its own diagonal: a band cell, the border (row 0 / the feed's column 0 while it is in
//          the band), or after a shift lane 0's X[0] / D[0] from before it, which was a band cell;
//        - the cell above it (x, j - 1), on diagonal x - j + 1 <= d_hi + 1: a band cell, or position g_e, just reset (rule 2);
//        - along the row what the gap_b scan carries: it runs left to right (wave_scan_span takes from lower lanes only, the
//          per-lane chain from lower c only), the band columns of a row are the frame's first n_row positions and position 0 is
//          fed by the feed cell; so a band cell sees band cells and the feed, never a position to its right.
//      A position right of the band on row j enters the band, if ever, by passing through g_e first: the right edge moves one
//      column per row and so does the frame from row -d_lo + 2 on; before that the edge walks over the positions one at a time.
//      There rule 2 resets all a band cell reads of it.  Columns right of len_a never enter the band.  Every add is addw.
//
// Every loop is bounded by the rows 1 .. len_b; no matrices, no hand-off, no waits but for the code fetches, no atomics but the
// err_flag OR.  The launches are recorded as "band_score" (the second launch record's table is pinned).
#include "sa_nw_stats.hpp"
#include "sa_band_pipe.hpp"   // frame_shift

namespace sa {

template <int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
band_nw_stats_rows_kernel(const SaBandNwStatsParams kp) {
  const SaBandParams &bp = kp.b;
  const SaFillParams &p = bp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  constexpr int F = kWave * CPL;
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t pair = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (pair >= p.n_pairs) return;   // wave-uniform, after the only barrier

  const uint32_t la = p.len_a[pair], lb = p.len_b[pair];
  const int d_lo = __builtin_amdgcn_readfirstlane(bp.d_lo[pair]);
  const int width = __builtin_amdgcn_readfirstlane((int)bp.width[pair]);
  const int d_hi = d_lo + width - 1;
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[pair];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[pair];
  const uint32_t W = la + 1;
  const SweepConsts k(p, table);
  const Border bd{p.floor, p.gap_open, p.ext, false, (p.flags & SA_F_NO_START_GAP) != 0};

  const int g0 = lane * CPL;   // my first frame position
  StatSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, bd, sa_, la, 0, (uint32_t)g0, lane);   // row 0's frame stands at column 1
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)

  // len_a == 0: the border column is the whole matrix
  const uint32_t rows = la ? lb : 0;
  int code_b = 0, code_in = 0;
  for (uint32_t j = 1; j <= rows; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {   // every 64 rows: lane t fetches seq_b's code for row j + t and the code of the column that enters on it
      const uint32_t r = j + lane;
      code_b = code_in = 0;
      if (r <= lb) {
        code_b = p.code[sb_[r - 1]];
        const long long idx = (long long)r + d_lo + F - 2;   // column fc(r) + F - 1, as an index into seq_a
        if ((long long)r + d_lo >= 2 && idx < (long long)la) code_in = p.code[sa_[idx]];
      }
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const int jd = (int)j + d_lo;          // <= len_a
    const int fc = max(1, jd);
    if (jd >= 2) {   // the frame moves (wave-uniform): rule 1
      const int cin = read_lane(code_in, q);
      sw.boundX = read_lane(sw.X[0], 0);
      sw.boundDm = (uint32_t)read_lane((int)sw.Dm[0], 0);
      sw.boundDn = (uint32_t)read_lane((int)sw.Dn[0], 0);
      frame_shift(sw.X, k.floor_);
      frame_shift(sw.Ap, k.floor_);
      if constexpr (GENERAL) frame_shift(sw.Y, k.floor_);
      frame_shift(sw.fa, cin & 0xff);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, (cin >> 8) * k.K);
      frame_shift(sw.Dm, 0u); frame_shift(sw.Dn, SA_STATS_NO_WALK);
      frame_shift(sw.Vm, 0u); frame_shift(sw.Vn, SA_STATS_NO_WALK);
    }
    // the cell above the band's right edge is outside the band: the floor, and no walk starts in it (rule 2)
    const int ge = (int)j + d_hi - fc - g0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? k.floor_ : sw.X[c];
      sw.Ap[c] = edge ? k.floor_ : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? k.floor_ : sw.Y[c];
      sw.Vm[c] = edge ? 0u : sw.Vm[c];
      sw.Vn[c] = edge ? SA_STATS_NO_WALK : sw.Vn[c];
      sw.Dm[c] = edge ? 0u : sw.Dm[c];
      sw.Dn[c] = edge ? SA_STATS_NO_WALK : sw.Dn[c];
    }
    const int n_row = min((int)la, (int)j + d_hi) - fc + 1;   // band columns of the row in the frame
    const int ncol = max(0, min(CPL, n_row - g0));
    const uint32_t col0 = (uint32_t)(fc - 1 + g0);
    // the cell left of the frame: the border column while it is in the band (NwStatsFamily::border_feed), else the floor in
    // both states and the mark in both payloads
    const bool border = jd <= 0;
    const StatFeed f{border ? max(k.floor_, bd.edge_gap(j)) : k.floor_, k.floor_, border ? 1 : 0, 0u, border ? 0u : SA_STATS_NO_WALK,
                     0u, border ? 0u : SA_STATS_NO_WALK};
    StatFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  if (la == 0) {   // cell (0, len_b) of the border column: in every band
    if (lane == 0) {
      bp.score[pair] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
      kp.matches[pair] = 0u; kp.mismatches[pair] = 0u;
    }
  } else {
    const int at = (int)la - max(1, (int)lb + d_lo) - g0;   // column len_a in the last row's frame
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      if (c == at) { bp.score[pair] = sw.X[c]; kp.matches[pair] = sw.Dm[c]; kp.mismatches[pair] = sw.Dn[c]; }
  }
  if (lane == 0) {
    p.status[pair] = err;
    if (err != ~0ull) atomicOr(bp.err_flag, 1u);
  }
}

template <int CPL>
static hipError_t launch_band_nw_stats_cpl(const SaBandNwStatsParams &p, hipStream_t stream) {
  const SaFillParams &f = p.b.f;
  const dim3 grid((f.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((band_nw_stats_rows_kernel<CPL, subst(), general()>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

hipError_t sa_launch_band_nw_stats(const SaBandNwStatsParams &p, uint32_t max_width, hipStream_t stream) {
  if (p.b.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_SPAN_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, p.b.f.n_pairs);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_width),
                                               [&](auto cpl) { return sa::launch_band_nw_stats_cpl<cpl()>(p, stream); });
}
