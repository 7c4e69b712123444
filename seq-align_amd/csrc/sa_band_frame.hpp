// sa_band_frame.hpp -- the moving frame of the banded SW payload sweeps, written once: band_payload_rows_kernel<P, CPL, SUBST,
// GENERAL> is the banded span kernel with P = BandSpanFrame (sa_band_span.hip: hit spans) and the banded statistics kernel
// with P = BandSwStatsFrame (sa_band_stats.hip: hit spans and identity counts), and launch_band_payload<P> their launch ladder.
// One wave per pair, 4 pairs per workgroup, a frame of F = 64 x CPL positions, CPL from {1 .. 6, 8} by the launch's widest band.
// Position g = lane * CPL + c holds column fc(j) + g on row j, fc(j) = max(1, j + d_lo).  The frame, its shift, the floor above
// the right edge and the rows swept are band_rows_kernel<.., FILL = false, SW = true>'s (sa_band.hip); the four rules of what
// the payloads do when the frame moves are stated in sa_band_span.hip's header, and each kernel file says what they mean for its
// two payload words.
//
// The family policy P is stateless.  It names the sweep (P::Sweep<CPL, SUBST, GENERAL>: SpanSweep or SwStatSweep, whose
// row<BAND = true> the shell calls) and its two payload words by role, so that the shell shifts, retires and resets them:
//   P::D0 / D1 / V0 / V1 (sw)         the diagonal and the vertical feed of the previous row (rule 1: they shift with X, Ap, Y,
//                                     fa, arow; rule 2: V of the cell above the right edge is reset to a stop);
//   P::boundD0 / boundD1 (sw)         the up-left of position 0 (rule 1: lane 0's D[0] from before the shift);
//   P::best0 / best1 (sw)             the words of the running best cell per position (rule 3: lane 0's retire, the rest shift);
//   P::stop0 / stop1 (x, y)           the two words of a cell (x, y) that holds 0 and stops the walk (rule 2: the edge cell, the
//                                     feed left of the frame);
//   P::first_row(sw, i0, col0, row)   the frame before the first row swept stands over zeros of row `row`: stops of their own;
//   P::write(kp, pair, score, key, words)   the pair's results from the best cell {score, (column << 32) | row, its two words}.
// The shell is the span kernel's former body statement for statement: the accessors are what keeps its instruction text (r23).
//
// The wide form (seqalign_sw_span_banded_wide, seqalign_sw_stats_banded_wide) is the second shell below,
// band_payload_strips_kernel<P, CPL, SUBST, GENERAL> with launch_band_payload_strips<P>, over the same policies: the same two
// families at any band width, one pair on many waves.  Two things that exist, crossed: the strip pipeline, the moving frame and
// the best cell merged from strip to strip of band_strips_kernel<CPL, SUBST, GENERAL, FILL = false, SW = true>
// (sa_band_strips.hip's header: the strips, their rows, the frame, the hand-off column, the tickets; sa_band_pipe.hpp: the
// bounded wait and the give-up word) and the four payload rules above around P::Sweep's row<BAND, PICK>.
// One workgroup = one wave = one (pair, strip), drawn by ticket.  Strip s owns columns c0 + 1 .. c0 + S, c0 = s S, S = 64 x CPL;
// its rows jf .. jl, fc(j) = max(c0 + 1, j + d_lo), fc_before = max(c0 + 1, d_lo), when the frame moves, ncol, left_rows /
// right_rows, the early exit of a strip without rows (strip 0 writes the zeros of a pair without inner band cells) and the
// progress, front and give-up words are band_strips_kernel's, to the letter.  The payload rules, as they read per strip:
//   Shift (rule 1).  D0 / D1 / V0 / V1 and bs / br / best0 / best1 shift with X, Ap, Y, fa, arow; boundX / boundD0 / boundD1
//     become lane 0's [0] from before the shift.  Lane 0's column retires into a wave-uniform best that keeps its two words
//     (strict >: a tie stays with the retired, lower column).  What enters on the right is a column past the strip's end, never
//     a cell of this strip: 0 in every word.
//   Outside the band is a stop (rule 2): 0 in all three states, its words P::stop0 / stop1 of the cell itself.  That is row
//     jf - 1 in all its columns (row 0 for jf = 1, which start_strip has written so; jf > 1 is written in the stop form, not
//     through P::first_row: 3.29); position g_e = j + d_hi - fc(j), the cell above the band's right edge, where it lies in the
//     frame, in X, Ap, Y, V0, V1 before every row; the feed left of the frame wherever (c0, j) is no band cell -- on every row
//     once the frame has moved, and strip 0's border column on all its rows -- which is {0, 0, not from A, stop (fc(j) - 1, j)
//     in both payloads}.
//   Left feed and up-left of a first row.  Strip s > 0, while (c0, j) is a band cell: the left strip's hand-off entry of the
//     row.  The up-left of a first row jf > 1 is (c0, jf - 1), on the band's right edge: hand-off entry 0, merged by row()'s
//     own boundary rule (A >= B > M via from_a).  Strip 0: the border cell (0, jf - 1), a stop of its own.
//   Hand-off.  Per row of the strip's last column c0 + S while that cell is in the band (rows c0 + S - d_hi .. c0 + S - d_lo):
//     StripSpanHandoff's content with x = word 0 and y = word 1, 32 bytes at entry [row - (c0 + S - d_hi)] of the strip's
//     `width` entries, moved 64 rows at a time and then published.  The column sits at frame position c0 + S - fc(j), which
//     moves: row<BAND, PICK> leaves that column's values in `out`, and they are read from the lane that holds it.
//   Best cell.  At the end of a strip reduce_best over the live columns, then the retired best first on a tie; then the wait for
//     the left strip's ~0 and merge_left_best_span (left wins a tie).  A strip with a right neighbour stores {score, end_a,
//     end_b, 0} {word 0, word 1, 0, 0} in its 32-byte best entry before its last publication, where the score kernel stores
//     its 16 bytes; the last strip of the run unpacks into the results through P::write.
// No band cell reads a frame position right of len_a or right of the strip's end c0 + S, whatever the sweep computes there (the
// statistics family needs this for its 16-bit coordinates: sa_band_stats.hip's header).  A band cell (x, j) of strip s, c0 < x
// <= min(len_a, c0 + S), reads exactly
//   - its up-left (x - 1, j - 1), on its own diagonal: a band cell of this strip, held one position to the left (frame standing)
//     or in the same position of the shifted arrays; for x = c0 + 1 the boundary, which row() derived from the feed of row
//     j - 1 (a band cell of the left strip or a stop in column c0 <= len_a), or the up-left rule above (hand-off entry 0, the
//     border cell, or start_strip's / the first-row stop (fc_before - 1, jf - 1), fc_before - 1 <= len_a); on the lowest diagonal
//     after a shift, lane 0's [0] from before the shift: the band cell (fc(j) - 1, j - 1) of this strip;
//   - the cell above it (x, j - 1), on diagonal x - j + 1 <= d_hi + 1: a band cell of this strip, or position g_e, which has just
//     been overwritten with the stop (j + d_hi, j - 1), and x = j + d_hi <= len_a there since (x, j) is a band cell; on the
//     strip's first row jf > 1 the stop (x, jf - 1) with x <= len_a;
//   - along the row, what the gap_b scan carries: left to right only (wave_scan_span takes from lower lanes, the per-lane chain
//     from lower c), and the strip's band columns of a row are the frame's FIRST n_row positions -- the frame starts on the
//     strip's first band column of the row and ends, for a band cell, at min(len_a, c0 + S, j + d_hi) -- with position 0 fed by
//     the feed, so a band cell sees band cells of this strip and the feed, never a position to its right;
//   - the feed: a hand-off entry, which is always a band cell's of the left strip (entries are stored only for rows on which
//     column c0 is in the band, and their words were exact there by this argument one strip to the left), or a stop in column
//     fc(j) - 1, and fc(j) - 1 <= len_a: fc(j) = c0 + 1 with c0 < len_a, or fc(j) = j + d_lo <= min(len_a, c0 + S) on the
//     strip's rows j <= jl.
// A position right of the band on row j enters the band, if ever, by passing through g_e first (the band's right edge moves one
// column per row; the frame moves one column per row or stands), where rule 2 resets everything a band cell reads of it: X, Ap,
// Y, V0, V1; its D0 / D1 are read only by the cell below-right of it, one diagonal further right and no band cell.  A position
// right of min(len_a, c0 + S) never holds a cell of this strip: it is masked out of the best cell and the error key by ncol,
// and the hand-off reads column c0 + S only where c0 + S < len_a (right_rows) and the cell is in the band.  So no mask is
// needed and none is applied.  Nothing waits on a strip to its right; every path out of the kernel publishes ~0; no loop is
// unbounded.
#pragma once
#include "sa_span.hpp"
#include "sa_band_pipe.hpp"

namespace sa {

template <class P, int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
band_payload_rows_kernel(const typename P::Params kp) {
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

  // the first row that has a band cell; the frame of the row before it stands at column max(1, d_lo), over zeros
  const uint32_t first = d_hi < 0 ? (uint32_t)(1 - d_hi) : 1u;
  const int g0 = lane * CPL;   // my first frame position
  typename P::template Sweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, sa_, la, (uint32_t)(max(1, d_lo) - 1), (uint32_t)(max(1, d_lo) - 1 + g0), lane);
  P::first_row(sw, (uint32_t)(max(1, d_lo) - 1), (uint32_t)(max(1, d_lo) - 1 + g0), first - 1);   // rule 2
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  // of the columns left of the frame (wave-uniform): best value, its column and first row, that cell's two words
  int ret_s = 0;
  uint32_t ret_col = 0, ret_row = 0, ret_0 = 0, ret_1 = 0;

  // len_a == 0: no inner cell.  Rows past the band's last cell are not swept
  const uint32_t rows = la ? min(lb, (uint32_t)((int)la - d_lo)) : 0;
  int code_b = 0, code_in = 0;
  for (uint32_t j = first; j <= rows; ++j) {
    const int q = (j - first) & (kWave - 1);
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
    if (jd >= 2) {   // the frame moves (wave-uniform): rules 1 and 3
      const int cin = read_lane(code_in, q);
      sw.boundX = read_lane(sw.X[0], 0);
      P::boundD0(sw) = (uint32_t)read_lane((int)P::D0(sw)[0], 0);
      P::boundD1(sw) = (uint32_t)read_lane((int)P::D1(sw)[0], 0);
      frame_shift(sw.X, 0);
      frame_shift(sw.Ap, 0);
      if constexpr (GENERAL) frame_shift(sw.Y, 0);
      frame_shift(sw.fa, cin & 0xff);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, (cin >> 8) * k.K);
      frame_shift(P::D0(sw), 0u); frame_shift(P::D1(sw), 0u);
      frame_shift(P::V0(sw), 0u); frame_shift(P::V1(sw), 0u);
      // column fc - 1 leaves through lane 0
      const int s0 = read_lane(sw.bs[0], 0);
      if (s0 > ret_s) {
        ret_s = s0; ret_col = (uint32_t)(fc - 1);
        ret_row = (uint32_t)read_lane((int)sw.br[0], 0);
        ret_0 = (uint32_t)read_lane((int)P::best0(sw)[0], 0);
        ret_1 = (uint32_t)read_lane((int)P::best1(sw)[0], 0);
      }
      frame_shift(sw.bs, 0);
      frame_shift(sw.br, 0u); frame_shift(P::best0(sw), 0u); frame_shift(P::best1(sw), 0u);
    }
    // the cell above the band's right edge is outside the band: 0, and a stop of its own (rule 2)
    const int ge = (int)j + d_hi - fc - g0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? 0 : sw.X[c];
      sw.Ap[c] = edge ? 0 : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? 0 : sw.Y[c];
      P::V0(sw)[c] = edge ? P::stop0((uint32_t)((int)j + d_hi), j - 1) : P::V0(sw)[c];
      P::V1(sw)[c] = edge ? P::stop1((uint32_t)((int)j + d_hi), j - 1) : P::V1(sw)[c];
    }
    const int n_row = min((int)la, (int)j + d_hi) - fc + 1;   // band columns of the row in the frame
    const int ncol = max(0, min(CPL, n_row - g0));
    const uint32_t col0 = (uint32_t)(fc - 1 + g0);
    // the cell left of the frame: the border column or a cell outside the band, 0 and a stop of its own either way
    const SpanFeed f{0, 0, 0, P::stop0((uint32_t)(fc - 1), j), P::stop1((uint32_t)(fc - 1), j), P::stop0((uint32_t)(fc - 1), j),
                     P::stop1((uint32_t)(fc - 1), j)};
    SpanFeed out;
    sw.template row<true>(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  int score;
  unsigned long long key, words;
  // the last row's frame (no row swept: every best is 0); a position that never held a band column has kept 0
  sw.reduce_best((uint32_t)(max(1, (int)rows + d_lo) - 1 + g0), CPL, score, key, words);
  if (ret_s >= score && ret_s > 0) {   // a tie goes to the lower column: a retired one
    score = ret_s;
    key = ((unsigned long long)ret_col << 32) | ret_row;
    words = ((unsigned long long)ret_0 << 32) | ret_1;
  }
  if (lane == 0) {
    P::write(kp, pair, score, key, words);
    p.status[pair] = err;
    if (err != ~0ull) atomicOr(bp.err_flag, 1u);
  }
}

template <class P, int CPL>
static hipError_t launch_band_payload_cpl(const typename P::Params &p, hipStream_t stream) {
  const SaFillParams &f = p.b.f;
  const dim3 grid((f.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((band_payload_rows_kernel<P, CPL, subst(), general()>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

// every pair of the launch has width <= max_width <= SA_SPAN_BAND_MAX_WIDTH; recorded as "band_score"
template <class P>
static hipError_t launch_band_payload(const typename P::Params &p, uint32_t max_width, hipStream_t stream) {
  if (p.b.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_SPAN_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, p.b.f.n_pairs);
  return launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(columns_per_lane(max_width), [&](auto cpl) { return launch_band_payload_cpl<P, cpl()>(p, stream); });
}

// ---- the wide form (header): one wave per (pair, strip)
template <class P, int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
band_payload_strips_kernel(const SaBandWideParams<typename P::Params> wp) {
  const typename P::Params &kp = wp.s;
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

  // my rows, and whether my neighbours have any (written out as in band_strips_kernel: a struct costs instructions, 3.29)
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

  if (!has_rows) {
    // no band cell in my columns.  A pair without any inner band cell gets its (empty) result from strip 0
    const long long colmin = max(1ll, 1ll + d_lo), colmax = min((long long)la, (long long)lb + d_hi);
    if (strip == 0 && (la == 0 || lb == 0 || colmin > colmax) && lane == 0) P::write(kp, pair, 0, ~0ull, 0ull);
    band_publish(word, front, kAllRows);
    return;
  }

  typename P::template Sweep<CPL, SUBST, GENERAL> sw;
  const int g0 = lane * CPL;   // my first frame position
  // the frame of the row before my first: on column max(c0 + 1, d_lo) (d_lo > c0 + 1 only where jf = 1)
  const int fc_before = (int)max(c0 + 1, (long long)d_lo);
  sw.start_strip(p, k, sa_, la, (uint32_t)(fc_before - 1), (uint32_t)(fc_before - 1 + g0), lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  if (jf > 1) {   // the row above my first is outside the band in all my columns: stops of their own (the values are 0 already)
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      P::D0(sw)[c] = P::V0(sw)[c] = P::stop0((uint32_t)(fc_before + g0 + c), (uint32_t)(jf - 1));
      P::D1(sw)[c] = P::V1(sw)[c] = P::stop1((uint32_t)(fc_before + g0 + c), (uint32_t)(jf - 1));
    }
    P::boundD0(sw) = P::stop0((uint32_t)(fc_before - 1), (uint32_t)(jf - 1));
    P::boundD1(sw) = P::stop1((uint32_t)(fc_before - 1), (uint32_t)(jf - 1));
  }
  // of my columns left of the frame (wave-uniform): best value, its column and first row, that cell's two words
  int ret_s = 0;
  uint32_t ret_col = 0, ret_row = 0, ret_0 = 0, ret_1 = 0;

  bool left_done = !left_rows;
  int code_b = 0;
  int4 in0 = {0, 0, 0, 0}, in1 = {0, 0, 0, 0};     // lane t: row j0 + t's feed from the left (StripSpanHandoff's entry)
  int4 out0 = {0, 0, 0, 0}, out1 = {0, 0, 0, 0};   // lane t: row j0 + t's entry of my last column
  const long long e_in0 = c0 - d_hi, e_out0 = c0 + F - d_hi;   // the rows of hand-off entry 0: in, out
  for (uint32_t j = (uint32_t)jf; j <= (uint32_t)jl; ++j) {
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
      {   // no band cell left of the frame (strip 0: the border column): 0, not an A's, a stop of its own
        const uint32_t sx = (uint32_t)(max(c0 + 1, (long long)r + d_lo) - 1);
        in0 = make_int4(0, 0, 0, 0);
        in1 = make_int4((int)P::stop0(sx, r), (int)P::stop1(sx, r), (int)P::stop0(sx, r), (int)P::stop1(sx, r));
      }
      if ((long long)r <= jl) {
        code_b = p.code[sb_[r - 1]];
        if (strip != 0) {
          const long long e = (long long)r - e_in0;
          if (e >= 0 && e < width) { in0 = hand_in[2 * e]; in1 = hand_in[2 * e + 1]; }
        }
      }
      if (j == (uint32_t)jf && jf > 1 && strip != 0) {   // the up-left of my first row: (c0, jf - 1), on the band's right edge
        const int4 h0 = hand_in[0], h1 = hand_in[1];
        const bool zwins = h0.z ? h0.x >= h0.y : h0.x > h0.y;
        sw.boundX = max(h0.x, h0.y);
        P::boundD0(sw) = (uint32_t)(zwins ? h1.x : h1.z);
        P::boundD1(sw) = (uint32_t)(zwins ? h1.y : h1.w);
      }
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const long long jd = (long long)j + d_lo;
    const int fc = (int)max(c0 + 1, jd);
    if (jd >= c0 + 2) {   // the frame moves (wave-uniform): rule 1
      sw.boundX = read_lane(sw.X[0], 0);
      P::boundD0(sw) = (uint32_t)read_lane((int)P::D0(sw)[0], 0);
      P::boundD1(sw) = (uint32_t)read_lane((int)P::D1(sw)[0], 0);
      frame_shift(sw.X, 0);
      frame_shift(sw.Ap, 0);
      if constexpr (GENERAL) frame_shift(sw.Y, 0);
      frame_shift(sw.fa, 0);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, 0);
      frame_shift(P::D0(sw), 0u); frame_shift(P::D1(sw), 0u);
      frame_shift(P::V0(sw), 0u); frame_shift(P::V1(sw), 0u);
      // column fc - 1 leaves through lane 0
      const int s0 = read_lane(sw.bs[0], 0);
      if (s0 > ret_s) {
        ret_s = s0; ret_col = (uint32_t)(fc - 1);
        ret_row = (uint32_t)read_lane((int)sw.br[0], 0);
        ret_0 = (uint32_t)read_lane((int)P::best0(sw)[0], 0);
        ret_1 = (uint32_t)read_lane((int)P::best1(sw)[0], 0);
      }
      frame_shift(sw.bs, 0);
      frame_shift(sw.br, 0u); frame_shift(P::best0(sw), 0u); frame_shift(P::best1(sw), 0u);
    }
    // the cell above the band's right edge is outside the band: 0, and a stop of its own (rule 2)
    const long long jh = (long long)j + d_hi;
    const int ge = (int)min(jh - fc, (long long)F) - g0;
    const uint32_t edge_0 = P::stop0((uint32_t)jh, j - 1), edge_1 = P::stop1((uint32_t)jh, j - 1);
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? 0 : sw.X[c];
      sw.Ap[c] = edge ? 0 : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? 0 : sw.Y[c];
      P::V0(sw)[c] = edge ? edge_0 : P::V0(sw)[c];
      P::V1(sw)[c] = edge ? edge_1 : P::V1(sw)[c];
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
    sw.template row<true, true>(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), f, out, pl % CPL);
    if (right_rows) {
      const int src = pl / CPL;
      const int z = read_lane(out.z, src), b = read_lane(out.b, src), za = read_lane(out.from_a, src);
      const int zx = read_lane((int)out.zx, src), zy = read_lane((int)out.zy, src);
      const int bx = read_lane((int)out.bx, src), by = read_lane((int)out.by, src);
      const bool mine = lane == q;   // (member by member: a select between two vectors may go through memory)
      out0 = make_int4(mine ? z : out0.x, mine ? b : out0.y, mine ? za : out0.z, 0);
      out1 = make_int4(mine ? zx : out1.x, mine ? zy : out1.y, mine ? bx : out1.z, mine ? by : out1.w);
      if (q == kWave - 1 || j == (uint32_t)jl) {
        // (a row on which my last column is right of the band, j + d_hi < c0 + F, has e < 0: its entry does not exist)
        const long long e = (long long)j - q + lane - e_out0;
        if (lane <= q && e >= 0 && e < width) { hand_out[2 * e] = out0; hand_out[2 * e + 1] = out1; }
        if (j != (uint32_t)jl) band_publish(word, front, j);   // (the last rows are published below, after the best cell)
      }
    }
  }

  const unsigned long long err = sw.reduce_err();
  if (lane == 0 && err != ~0ull) {
    atomicMin(reinterpret_cast<unsigned long long *>(p.status + pair), err);
    atomicOr(bp.err_flag, 1u);
  }
  int score;
  unsigned long long key, words;
  // the last row's frame; a position that never held a band column of mine has kept 0
  sw.reduce_best((uint32_t)((int)max(c0 + 1, jl + d_lo) - 1 + g0), CPL, score, key, words);
  if (ret_s >= score && ret_s > 0) {   // a tie goes to the lower column: a retired one
    score = ret_s;
    key = ((unsigned long long)ret_col << 32) | ret_row;
    words = ((unsigned long long)ret_0 << 32) | ret_1;
  }
  const uint64_t slot = wp.w.slot_off[pair] + strip;
  if (left_rows) {   // the best of the strips to my left: written before that strip's last publication
    if (!band_strip_wait(word - 1, front, kAllRows)) {
      band_give_up(wp.w.give_up, pair, word, front);
      return;
    }
    merge_left_best_span(wp.w.strip_best + kSpanBestWords * (slot - 1), score, key, words);
  }
  if (lane == 0) {
    if (!right_rows) {
      P::write(kp, pair, score, key, words);
    } else {
      const uint32_t ea = score > 0 ? (uint32_t)(key >> 32) : 0u, eb = score > 0 ? (uint32_t)key : 0u;
      uint4 *entry = reinterpret_cast<uint4 *>(wp.w.strip_best + kSpanBestWords * slot);
      entry[0] = make_uint4((uint32_t)score, ea, eb, 0u);
      entry[1] = make_uint4((uint32_t)(words >> 32), (uint32_t)words, 0u, 0u);
    }
  }
  band_publish(word, front, kAllRows);
}

// strip_cols: 64 | 128 | 256 | 512; recorded as "band_score" with `items`
template <class P>
static hipError_t launch_band_payload_strips(const SaBandWideParams<typename P::Params> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  const SaFillParams &f = p.s.b.f;
  if (f.n_pairs == 0) return hipSuccess;
  dim3 grid;
  if (band_strips_grid(f.n_pairs, p.w.strips_per_pair, grid) != hipSuccess) return hipErrorInvalidValue;
  return launch_by_strip_cols(strip_cols, [&](auto cpl) {
    sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items);
    launch_by_scoring(f, [&](auto subst, auto general, uint32_t table_ints) {
      hipLaunchKernelGGL((band_payload_strips_kernel<P, cpl(), subst(), general()>), grid, dim3(kWave), table_ints * sizeof(int32_t), stream, p);
    });
    return hipGetLastError();
  });
}

}  // namespace sa
