// sa_band_nw_stats_strips.hip -- wide banded NW statistics (seqalign_nw_stats_banded_wide): seqalign_nw_stats_banded's three
// integers at any band width, one pair on many waves.  Two things that exist, crossed: the strip pipeline and moving frame of
// band_strips_kernel<CPL, SUBST, GENERAL, FILL = false, SW = false> (sa_band_strips.hip's header: the strips, their rows, the
// frame, the hand-off column and the tickets; the bounded wait and the give-up word: sa_band_pipe.hpp) and the payload rules of
// band_nw_stats_rows_kernel (sa_band_nw_stats.hip's header: the mark, the four rules) around StatSweep::row.  DESIGN.md 3.26.
//
// band_nw_stats_strips_kernel<CPL, SUBST, GENERAL>: one workgroup = one wave = one (pair, strip), drawn by ticket.  Strip s owns
// columns c0 + 1 .. c0 + S, c0 = s S, S = 64 x CPL; its rows jf .. jl, fc(j) = max(c0 + 1, j + d_lo), when the frame moves, ncol,
// left_rows / right_rows and the progress, front and give-up words are band_strips_kernel's, to the letter.  The payload rules,
// as they read per strip:
//   Shift (rule 1).  Dm / Dn / Vm / Vn shift with X, Ap, Y, fa, arow; boundX / boundDm / boundDn become lane 0's [0] from before
//     the shift.  What enters on the right is a column past the strip's end, never a cell of this strip: the floor and the mark.
//   The cell above the right edge (rule 2).  Position g_e = j + d_hi - fc(j), where it lies in the frame, gets the floor in X, Ap,
//     Y and the mark in Vm / Vn AND Dm / Dn before every row.  A strip whose first row is jf > 1 starts with the floor and the
//     mark in every position: row jf - 1 is outside the band in all its columns.
//   Left feed while the frame stands.  Strip 0: NwStatsFamily::border_feed's values while the border column is in the band
//     (j <= -d_lo).  Strip s > 0: the left strip's hand-off entry of the row.  Where the entry does not exist -- (c0, j) is outside
//     the band, which is also so on every row of the moving phase -- the floor, the mark and from_a = 0.  StatSweep::row derives
//     the next row's boundX / boundDm / boundDn from the feed; the moving phase overwrites them (rule 1).
//   Up-left of a strip's first row (jf > 1, s > 0): cell (c0, jf - 1), hand-off entry 0: boundX = max(z, b), boundDm / boundDn by
//     row()'s boundary rule with `forced` as it holds on row jf - 1.
//   Hand-off.  Per row of the strip's last column c0 + S while that cell is in the band (rows c0 + S - d_hi .. c0 + S - d_lo):
//     max(M, A), B, whether max(M, A) is an admitted A's, and the two payloads -- StripSpanHandoff's content, 32 bytes at entry
//     [row - (c0 + S - d_hi)] of the strip's `width` entries, moved 64 rows at a time and then published.  The column sits at
//     frame position c0 + S - fc(j), which moves: StatSweep::row<PICK> leaves that column's values in `out`, and they are read
//     from the lane that holds it.
//   Result.  The last strip writes X, Dm, Dn of column len_a in the last row's frame; len_a = 0: strip 0 writes the border cell
//     and (0, 0).  Status: atomicMin of the lowest band cell without a score.
// So a band cell reads what it reads in the narrow kernel (rule 4 there) and besides only the feed, which is a band cell of the
// left strip or the floor and the mark.  Nothing waits on a strip to its right; every path out of the kernel publishes ~0.
#include "sa_nw_stats.hpp"
#include "sa_band_pipe.hpp"

namespace sa {

template <int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
band_nw_stats_strips_kernel(const SaBandWideParams<SaBandNwStatsParams> wp) {
  const SaBandNwStatsParams &kp = wp.s;
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

  StatSweep<CPL, SUBST, GENERAL> sw;
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
        if (strip == 0) {   // the border column while it is in the band: NwStatsFamily::border_feed
          if ((long long)r <= -(long long)d_lo) {
            in0 = make_int4(max(k.floor_, bd.edge_gap(r)), k.floor_, 1, 0);
            in1 = make_int4(0, 0, 0, 0);
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
    const StatFeed f{read_lane(in0.x, q), read_lane(in0.y, q), read_lane(in0.z, q),
                     (uint32_t)read_lane(in1.x, q), (uint32_t)read_lane(in1.y, q),
                     (uint32_t)read_lane(in1.z, q), (uint32_t)read_lane(in1.w, q)};
    // my last column, c0 + F (<= len_a where anyone reads it), at frame position c0 + F - fc
    const int pl = (int)(c0 + F - fc);
    StatFeed out{};
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
      kp.matches[pair] = 0u; kp.mismatches[pair] = 0u;
    }
  } else if (c0 + F >= (long long)la) {   // the last strip: column len_a in the last row's frame
    const int at = (int)((long long)la - max(c0 + 1, (long long)lb + d_lo)) - g0;
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      if (c == at) { bp.score[pair] = sw.X[c]; kp.matches[pair] = sw.Dm[c]; kp.mismatches[pair] = sw.Dn[c]; }
  }
  band_publish(word, front, kAllRows);
}

}  // namespace sa

hipError_t sa_launch_band_nw_stats_strips(const SaBandWideParams<SaBandNwStatsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  if (p.s.b.f.n_pairs == 0) return hipSuccess;
  dim3 grid;
  if (sa::band_strips_grid(p.s.b.f.n_pairs, p.w.strips_per_pair, grid) != hipSuccess) return hipErrorInvalidValue;
  return sa::launch_by_strip_cols(strip_cols, [&](auto cpl) {
    sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items);
    sa::launch_by_scoring(p.s.b.f, [&](auto subst, auto general, uint32_t table_ints) {
      hipLaunchKernelGGL((sa::band_nw_stats_strips_kernel<cpl(), subst(), general()>), grid, dim3(sa::kWave), table_ints * sizeof(int32_t), stream, p);
    });
    return hipGetLastError();
  });
}
