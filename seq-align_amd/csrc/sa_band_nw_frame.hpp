// sa_band_nw_frame.hpp -- the NW band frame of the payload sweeps: the two kernel shells that carry a two-word payload with the
// NW mark through a band of diagonals, over a small family.  band_nw_payload_rows_kernel is the narrow kernel (one wave per
// pair, at most 512 diagonals), band_nw_payload_strips_kernel the wide one (one wave per pair and strip, any width).  Their
// families are the banded NW statistics (sa_band_nw_stats.hip, sa_band_nw_stats_strips.hip: matches and mismatches, StatSweep)
// and the banded NW gap-run counts (sa_band_nw_gaps.hip: gap_runs_a and gap_runs_b, NwGapSweep).  DESIGN.md 3.25, 3.26, 3.34.
// A family is a policy B: types, constants and static device functions, no state.  It names
//   Params                      the narrow launch's parameter block: SaBandNwStatsParams or a typedef of it
//   Sweep<CPL, SUBST, GENERAL>  its sweep: StatSweep's members by StatSweep's names -- Dm / Dn and Vm / Vn, the diagonal and the
//                               vertical feed's word 0 and word 1 (word 1 holds the mark), boundDm / boundDn, the diagonal feed
//                               of the cell left of the frame on the previous row -- and row<PICK>.  (The frame names the
//                               members itself: reached through accessors of the family the statistics kernels' text changed.)
//   kBorderX                    word 0 of a cell (0, y), y > 0, of the border column in both of its payloads; word 1 is 0 there.
//                               (Row 0 is the sweep's own start_strip.)  It is also word 0 of the result of a pair with
//                               len_a = 0 < len_b, whose word 1 is 0.
// Nothing else differs between the families: the floor and the mark outside the band, the reset above the right edge and the
// three phases of the left feed are the frame's.
//
// The narrow kernel, band_nw_payload_rows_kernel<B, CPL, SUBST, GENERAL>: the sweep's row arithmetic inside the NW frame of
// band_rows_kernel<.., SW = false> (sa_band.hip's header: the frame, the three phases of the feed, why the band's edges are
// exact).  One wave per pair, 4 pairs per workgroup, a frame of F = 64 x CPL positions, CPL from {1 .. 6, 8} by the launch's
// widest band.  Position g = lane * CPL + c holds column fc(j) + g on row j, fc(j) = max(1, j + d_lo), d_lo <= 0 <= d_hi.  A
// sibling of band_payload_rows_kernel (sa_band_frame.hpp, the SW payload frame) that shares frame_shift (sa_band_pipe.hpp) with
// it and nothing else; what differs from the SW frame:
//   No best cell, no retire.  Both corners are in every NW band, so every row 1 .. len_b is swept and the result is the last
//   row's position len_a - fc(len_b): its X and its diagonal feed Dm / Dn, the end pick's payload as in StatSweep::write.
//   A cell outside the band is no stop.  It holds the floor in all three states, and a state at the floor with no candidate has
//   no walk: its payload is the sticky mark (0, SA_STATS_NO_WALK), never the border's.  A band cell whose best candidate is such
//   a cell either stays below the floor itself (then the sweep's row marks it) or carries the mark on from the feed.
// The four rules of payloads in a moving frame (sa_band_span.hip's header), as they read here:
//   1. The shift.  From row -d_lo + 2 on the frame moves one column per row: Dm / Dn / Vm / Vn shift left by one position with
//      X, Ap, Y, fa, arow, and boundX / boundDm / boundDn become lane 0's X[0] / Dm[0] / Dn[0] from before the shift: cell
//      (fc(j) - 1, j - 1), on the band's lowest diagonal.  What enters on the right is column fc(j) + F - 1 of row j - 1, on
//      diagonal d_lo + F > d_hi: outside the band, the floor and the mark.
//   2. The floor outside the band.  The feed left of the frame has three phases.  Rows j <= -d_lo: the border column is in the
//      band and the feed is the unbanded kernel's border feed (gap_a holds the edge, the border's payload, no mark).  Row
//      -d_lo + 1: the feed cell (0, j) is outside the band -- the floor and the mark in both of its payloads -- and the frame
//      does not move yet; the up-left of position 0 is still the border cell (0, -d_lo), which the sweep's row kept from the
//      previous row's feed (or cell (0, 0) from start_strip when d_lo = 0).  From row -d_lo + 2 on: the same feed, and rule 1
//      overwrites what row() derived from it for the up-left.
//      The cell above the right edge -- position g_e = j + d_hi - fc(j), column j + d_hi of row j - 1 -- is read two ways by the
//      band cell below it: through V (gap_a: Y, Ap, Vm, Vn), and, under no_end_gap_penalty in the last column, through D
//      (a_free takes max(Y, Ap) and Dm[c] / Dn[c] of its own position).  So before row j position g_e gets the floor in X, Ap, Y
//      and the mark in Vm / Vn AND in Dm / Dn.  Resetting D there harms no band cell: D of position g_e is read by that a_free
//      cell, which must see the mark, and otherwise only as the up-left of the cell below-right of it, (j + d_hi + 1, j), on
//      diagonal d_hi + 1: one diagonal outside the band.
//      Row 0 is the sweep's start_strip's border: columns 1 .. d_hi are band cells (the edge gap, the border's payload); column
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
// Every loop is bounded by the rows 1 .. len_b; no matrices, no hand-off, no waits but for the code fetches, no atomics but the
// err_flag OR.
//
// The wide kernel, band_nw_payload_strips_kernel<B, CPL, SUBST, GENERAL>: two things that exist, crossed: the strip pipeline and
// moving frame of band_strips_kernel<CPL, SUBST, GENERAL, FILL = false, SW = false> (sa_band_strips.hip's header: the strips,
// their rows, the frame, the hand-off column and the tickets; the bounded wait and the give-up word: sa_band_pipe.hpp) and the
// payload rules above.  One workgroup = one wave = one (pair, strip), drawn by ticket.  Strip s owns columns c0 + 1 .. c0 + S,
// c0 = s S, S = 64 x CPL; its rows jf .. jl, fc(j) = max(c0 + 1, j + d_lo), when the frame moves, ncol, left_rows / right_rows
// and the progress, front and give-up words are band_strips_kernel's, to the letter.  The payload rules, as they read per strip:
//   Shift (rule 1).  Dm / Dn / Vm / Vn shift with X, Ap, Y, fa, arow; boundX / boundDm / boundDn become lane 0's [0] from before
//     the shift.  What enters on the right is a column past the strip's end, never a cell of this strip: the floor and the mark.
//   The cell above the right edge (rule 2).  Position g_e = j + d_hi - fc(j), where it lies in the frame, gets the floor in X, Ap,
//     Y and the mark in Vm / Vn AND Dm / Dn before every row.  A strip whose first row is jf > 1 starts with the floor and the
//     mark in every position: row jf - 1 is outside the band in all its columns.
//   Left feed while the frame stands.  Strip 0: the border column's values while it is in the band (j <= -d_lo).  Strip s > 0:
//     the left strip's hand-off entry of the row.  Where the entry does not exist -- (c0, j) is outside the band, which is also
//     so on every row of the moving phase -- the floor, the mark and from_a = 0.  The sweep's row derives the next row's boundX /
//     boundDm / boundDn from the feed; the moving phase overwrites them (rule 1).
//   Up-left of a strip's first row (jf > 1, s > 0): cell (c0, jf - 1), hand-off entry 0: boundX = max(z, b), boundDm / boundDn by
//     row()'s boundary rule with `forced` as it holds on row jf - 1.
//   Hand-off.  Per row of the strip's last column c0 + S while that cell is in the band (rows c0 + S - d_hi .. c0 + S - d_lo):
//     max(M, A), B, whether max(M, A) is an admitted A's, and the two payloads -- StripSpanHandoff's content, 32 bytes at entry
//     [row - (c0 + S - d_hi)] of the strip's `width` entries, moved 64 rows at a time and then published.  The column sits at
//     frame position c0 + S - fc(j), which moves: the sweep's row<PICK> leaves that column's values in `out`, and they are read
//     from the lane that holds it.
//   Result.  The last strip writes X, Dm, Dn of column len_a in the last row's frame; len_a = 0: strip 0 writes the border cell
//     and its payload.  Status: atomicMin of the lowest band cell without a score.
// So a band cell reads what it reads in the narrow kernel (rule 4) and besides only the feed, which is a band cell of the left
// strip or the floor and the mark.  Nothing waits on a strip to its right; every path out of the kernel publishes ~0.
// The launches are recorded as "band_score" (the second launch record's table is pinned).
#pragma once
#include "sa_span.hpp"
#include "sa_band_pipe.hpp"   // frame_shift, the strips' waits and publishes

namespace sa {

template <class B, int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
band_nw_payload_rows_kernel(const typename B::Params kp) {
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
  typename B::template Sweep<CPL, SUBST, GENERAL> sw;
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
    // the cell left of the frame: the border column while it is in the band (the unbanded family's border_feed), else the floor
    // in both states and the mark in both payloads
    const bool border = jd <= 0;
    const SpanFeed f{border ? max(k.floor_, bd.edge_gap(j)) : k.floor_, k.floor_, border ? 1 : 0,
                     border ? B::kBorderX : 0u, border ? 0u : SA_STATS_NO_WALK,
                     border ? B::kBorderX : 0u, border ? 0u : SA_STATS_NO_WALK};
    SpanFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  if (la == 0) {   // cell (0, len_b) of the border column: in every band
    if (lane == 0) {
      bp.score[pair] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
      kp.matches[pair] = lb == 0 ? 0u : B::kBorderX; kp.mismatches[pair] = 0u;
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

template <class B, int CPL>
static hipError_t launch_band_nw_payload_cpl(const typename B::Params &p, hipStream_t stream) {
  const SaFillParams &f = p.b.f;
  const dim3 grid((f.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((band_nw_payload_rows_kernel<B, CPL, subst(), general()>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

// every pair of the launch has width <= max_width <= SA_SPAN_BAND_MAX_WIDTH; max_width picks the columns per lane
template <class B>
hipError_t launch_band_nw_payload(const typename B::Params &p, uint32_t max_width, hipStream_t stream) {
  if (p.b.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_SPAN_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, p.b.f.n_pairs);
  return launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(columns_per_lane(max_width),
                                           [&](auto cpl) { return launch_band_nw_payload_cpl<B, cpl()>(p, stream); });
}

template <class B, int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
band_nw_payload_strips_kernel(const SaBandWideParams<typename B::Params> wp) {
  const typename B::Params &kp = wp.s;
  const SaBandParams &bp = kp.b;
  const SaFillParams &p = bp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  constexpr int F = kWave * CPL;   // the strip's columns, and the frame's positions
  const int lane = threadIdx.x;
  uint32_t strip, pair;
  strip_of_ticket(strip_ticket(wp.w.ticket), wp.w.strips_per_pair, strip, pair);
  if (pair >= p.n_pairs) return;

  const uint32_t la = p.len_a[pair], lb = p.len_b[pair];
  const long long c0 = (long long)strip * F;
  if (c0 >= (long long)la && strip != 0) return;   // this pair has fewer strips: no progress word, nobody waits for it
  uint32_t *word = wp.w.progress + wp.w.slot_off[pair] + strip;
  uint32_t *front = wp.w.front + pair;   // publications by any strip of the pair

  const int d_lo = __builtin_amdgcn_readfirstlane(bp.d_lo[pair]);
  const int width = __builtin_amdgcn_readfirstlane((int)bp.width[pair]);
  const int d_hi = d_lo + width - 1;
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[pair];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[pair];
  const uint32_t W = la + 1;

  const SweepConsts k(p, table);
  const Border bd{p.floor, p.gap_open, p.ext, false, (p.flags & SA_F_NO_START_GAP) != 0};

  // my rows, and whether my neighbours have any
  const long long cend = min((long long)la, c0 + F);
  const long long jf = max(1ll, c0 + 1 - d_hi), jl = la ? min((long long)lb, cend - d_lo) : 0;
  const bool has_rows = jf <= jl;
  const long long jl_left = min((long long)lb, c0 - d_lo);   // the left strip's last row
  const bool left_rows = strip > 0 && jl_left >= 1;
  const bool right_rows = lb >= 1 && c0 + F < (long long)la && c0 + F + 1 <= (long long)lb + d_hi;

  // entry e of a strip's hand-off column: two int4 at [2 e]
  const uint64_t hbase = wp.w.hand_off[pair];
  int4 *hand_out = reinterpret_cast<int4 *>(wp.w.handoff) + 2 * (hbase + (uint64_t)strip * (uint32_t)width);
  const int4 *hand_in = reinterpret_cast<const int4 *>(wp.w.handoff) + 2 * (hbase + (uint64_t)(strip ? strip - 1 : 0) * (uint32_t)width);

  typename B::template Sweep<CPL, SUBST, GENERAL> sw;
  const int g0 = lane * CPL;   // my first frame position
  sw.start_strip(p, k, bd, sa_, la, (uint32_t)c0, (uint32_t)(c0 + g0), lane);   // row 0's frame stands at column c0 + 1
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  if (jf > 1) {   // the row above my first is outside the band in all my columns
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      sw.X[c] = k.floor_;
      sw.Ap[c] = k.floor_;
      if constexpr (GENERAL) sw.Y[c] = k.floor_;
      sw.Dm[c] = sw.Vm[c] = 0u;
      sw.Dn[c] = sw.Vn[c] = SA_STATS_NO_WALK;
    }
  }

  bool left_done = !left_rows;
  int code_b = 0;
  int4 in0 = {0, 0, 0, 0}, in1 = {0, 0, 0, 0};     // lane t: row j0 + t's feed from the left (StripSpanHandoff's entry)
  int4 out0 = {0, 0, 0, 0}, out1 = {0, 0, 0, 0};   // lane t: row j0 + t's entry of my last column
  const long long e_in0 = c0 - d_hi, e_out0 = c0 + F - d_hi;   // the rows of hand-off entry 0: in, out
  for (uint32_t j = (uint32_t)jf; has_rows && j <= (uint32_t)jl; ++j) {
    const int q = (j - (uint32_t)jf) & (kWave - 1);
    if (q == 0) {
      if (!left_done) {   // rows j .. j + 63 of the strip to my left, as far as it has rows
        const uint32_t need = (uint32_t)min((long long)j + kWave - 1, jl_left);
        if (!band_strip_wait(word - 1, front, need)) {
          band_give_up(wp.w.give_up, pair, word, front);
          return;
        }
        left_done = (long long)need >= jl_left;
      }
      const uint32_t r = j + lane;
      code_b = 0;
      in0 = make_int4(k.floor_, k.floor_, 0, 0);   // no cell left of the frame: the floor, the mark, not an A's
      in1 = make_int4(0, (int)SA_STATS_NO_WALK, 0, (int)SA_STATS_NO_WALK);
      if ((long long)r <= jl) {
        code_b = p.code[sb_[r - 1]];
        if (strip == 0) {   // the border column while it is in the band: the unbanded family's border_feed
          if ((long long)r <= -(long long)d_lo) {
            in0 = make_int4(max(k.floor_, bd.edge_gap(r)), k.floor_, 1, 0);
            in1 = make_int4((int)B::kBorderX, 0, (int)B::kBorderX, 0);
          }
        } else {
          const long long e = (long long)r - e_in0;
          if (e >= 0 && e < width) { in0 = hand_in[2 * e]; in1 = hand_in[2 * e + 1]; }
        }
      }
      if (j == (uint32_t)jf && jf > 1) {   // the up-left of my first row: (c0, jf - 1), on the band's right edge
        sw.boundX = k.floor_; sw.boundDm = 0u; sw.boundDn = SA_STATS_NO_WALK;
        if (strip != 0) {
          const int4 h0 = hand_in[0], h1 = hand_in[1];
          const bool forced = GENERAL && k.no_gaps_b && (long long)lb != jf - 1;
          const bool zwins = forced || (h0.z ? h0.x >= h0.y : h0.x > h0.y);
          sw.boundX = max(h0.x, h0.y);
          sw.boundDm = (uint32_t)(zwins ? h1.x : h1.z);
          sw.boundDn = (uint32_t)(zwins ? h1.y : h1.w);
        }
      }
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const long long jd = (long long)j + d_lo;
    const int fc = (int)max(c0 + 1, jd);
    if (jd >= c0 + 2) {   // the frame moves (wave-uniform): rule 1
      sw.boundX = read_lane(sw.X[0], 0);
      sw.boundDm = (uint32_t)read_lane((int)sw.Dm[0], 0);
      sw.boundDn = (uint32_t)read_lane((int)sw.Dn[0], 0);
      frame_shift(sw.X, k.floor_);
      frame_shift(sw.Ap, k.floor_);
      if constexpr (GENERAL) frame_shift(sw.Y, k.floor_);
      frame_shift(sw.fa, 0);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, 0);
      frame_shift(sw.Dm, 0u); frame_shift(sw.Dn, SA_STATS_NO_WALK);
      frame_shift(sw.Vm, 0u); frame_shift(sw.Vn, SA_STATS_NO_WALK);
    }
    // the cell above the band's right edge is outside the band: the floor, and no walk starts in it (rule 2)
    const long long jh = (long long)j + d_hi;
    const int ge = (int)min(jh - fc, (long long)F) - g0;
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
    const int n_row = (int)(min(cend, jh) - fc + 1);   // my band columns of the row
    const int ncol = max(0, min(CPL, n_row - g0));
    const uint32_t col0 = (uint32_t)(fc - 1 + g0);
    const SpanFeed f{read_lane(in0.x, q), read_lane(in0.y, q), read_lane(in0.z, q),
                     (uint32_t)read_lane(in1.x, q), (uint32_t)read_lane(in1.y, q),
                     (uint32_t)read_lane(in1.z, q), (uint32_t)read_lane(in1.w, q)};
    // my last column, c0 + F (<= len_a where anyone reads it), at frame position c0 + F - fc
    const int pl = (int)(c0 + F - fc);
    SpanFeed out{};
    sw.template row<true>(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), f, out, pl % CPL);
    if (right_rows) {
      const bool inb = jh >= c0 + F;   // (its lower edge j + d_lo <= c0 + F holds on all my rows)
      const int src = pl / CPL;
      const int z = inb ? read_lane(out.z, src) : k.floor_, b = inb ? read_lane(out.b, src) : k.floor_;
      const int za = inb ? read_lane(out.from_a, src) : 0;
      const int zx = inb ? read_lane((int)out.zx, src) : 0, zy = inb ? read_lane((int)out.zy, src) : (int)SA_STATS_NO_WALK;
      const int bx = inb ? read_lane((int)out.bx, src) : 0, by = inb ? read_lane((int)out.by, src) : (int)SA_STATS_NO_WALK;
      const bool mine = lane == q;   // (member by member: a select between two vectors may go through memory)
      out0 = make_int4(mine ? z : out0.x, mine ? b : out0.y, mine ? za : out0.z, 0);
      out1 = make_int4(mine ? zx : out1.x, mine ? zy : out1.y, mine ? bx : out1.z, mine ? by : out1.w);
      if (q == kWave - 1 || j == (uint32_t)jl) {
        const long long e = (long long)j - q + lane - e_out0;
        if (lane <= q && e >= 0 && e < width) { hand_out[2 * e] = out0; hand_out[2 * e + 1] = out1; }
        if (j != (uint32_t)jl) band_publish(word, front, j);   // (the last rows are published below)
      }
    }
  }

  const unsigned long long err = sw.reduce_err();
  if (lane == 0 && err != ~0ull) {
    atomicMin(reinterpret_cast<unsigned long long *>(p.status + pair), err);
    atomicOr(bp.err_flag, 1u);
  }
  if (la == 0) {   // cell (0, len_b) of the border column
    if (lane == 0) {
      bp.score[pair] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
      kp.matches[pair] = lb == 0 ? 0u : B::kBorderX; kp.mismatches[pair] = 0u;
    }
  } else if (c0 + F >= (long long)la) {   // the last strip: column len_a in the last row's frame
    const int at = (int)((long long)la - max(c0 + 1, (long long)lb + d_lo)) - g0;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      if (c == at) { bp.score[pair] = sw.X[c]; kp.matches[pair] = sw.Dm[c]; kp.mismatches[pair] = sw.Dn[c]; }
  }
  band_publish(word, front, kAllRows);
}

template <class B>
hipError_t launch_band_nw_payload_strips(const SaBandWideParams<typename B::Params> &p, uint32_t strip_cols, uint64_t items,
                                         hipStream_t stream) {
  if (p.s.b.f.n_pairs == 0) return hipSuccess;
  dim3 grid;
  if (band_strips_grid(p.s.b.f.n_pairs, p.w.strips_per_pair, grid) != hipSuccess) return hipErrorInvalidValue;
  return launch_by_strip_cols(strip_cols, [&](auto cpl) {
    sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items);
    launch_by_scoring(p.s.b.f, [&](auto subst, auto general, uint32_t table_ints) {
      hipLaunchKernelGGL((band_nw_payload_strips_kernel<B, cpl(), subst(), general()>), grid, dim3(kWave), table_ints * sizeof(int32_t), stream, p);
    });
    return hipGetLastError();
  });
}

}  // namespace sa
