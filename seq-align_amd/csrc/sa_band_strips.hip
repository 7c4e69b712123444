// sa_band_strips.hip -- the wide banded calls (seqalign_*_banded_wide): the moving frame of band_rows_kernel (sa_band.hip), run
// per column strip by a pipeline of waves (sa_strips.hpp), so that a band may be any number of diagonals wide and one pair
// may occupy many waves.  The band, the matrices and the layouts are the narrow calls' (include/seqalign_hip.h).
//
// band_strips_kernel: one workgroup = one wave = one (pair, strip), drawn by ticket exactly as in score_strips_kernel: a
//   strip's ticket is above its left neighbour's, so the only wave a strip ever waits for -- the strip to its LEFT -- is
//   resident or done.  Nothing waits on a strip to its right.
//   Strip s owns columns c0 + 1 .. c0 + S, c0 = s S, S = 64 x CPL (CPL 1 / 2 / 4 / 8).  It sweeps only the rows on which one
//   of its columns is in the band: jf = max(1, c0 + 1 - d_hi) .. jl = min(len_b, min(len_a, c0 + S) - d_lo) (for SW that is
//   already inside sa_band_sw_rows' range).  A strip without such a row does nothing and publishes at once.
//   Frame.  On row j the frame's first column is fc(j) = max(c0 + 1, j + d_lo): it stands on the strip's first column until
//   the band's left edge enters the strip, then moves one column per row -- band_rows_kernel's frame_shift of X / Ap / Y /
//   fa / arow, boundX = lane 0's X[0] from before the shift.  What enters on the right is a column past the strip's end: it
//   is never a cell of this strip (ncol, the lane's count of the strip's band columns on the row, shrinks as the frame runs
//   into the strip's fixed right end), so it needs no code and gets the floor.  The position above the band's right edge
//   gets the floor before every row, as in band_rows_kernel, whatever the sweep left there.
//   Left feed.  While the frame stands, the cell left of it is column c0: the border column for strip 0 while that is in
//   the band (NW), strip s - 1's hand-off for that row otherwise; the hand-off holds the floor where (c0, j) is outside the
//   band, and once the frame has moved (j + d_lo > c0 + 1) the row's hand-off entry does not exist: the floor.  The up-left
//   of a strip's first row comes from the same hand-off (row jf - 1 = c0 - d_hi, on the band's right edge) or is the border.
//   So no band cell ever reads a computed cell that lies outside the band, and every exactness argument of sa_band.hip's
//   header holds per strip: nothing is masked in the middle of a row.
//   Hand-off.  Per row, max(M, A) and B of the strip's LAST column c0 + S when that cell is in the band -- rows c0 + S - d_hi
//   .. c0 + S - d_lo, the only ones the right strip reads -- 8 bytes at [row - (c0 + S - d_hi)] of the strip's hand-off
//   column of `width` entries, moved 64 rows at a time and then published (the row number) in the strip's progress word.
//   A waiter asks for min(j + 63, the left strip's last row); every strip that has a progress word publishes ~0, "all my
//   rows", on every path out of the kernel.
//   SW.  BandBest per frame position as in band_rows_kernel; the strips that have rows form one run, each merges the best
//   of the strips to its left (a tie stays left: lower columns) after waiting for that strip's ~0, and the last of the run
//   writes the pair's result.  A pair none of whose strips has a row gets score 0 from strip 0.
//   NW border cells of the fill form are written by strip 0, up front.
//   The wait is sa_band_pipe.hpp's band_strip_wait, bounded, with its give-up path (that header: the budget and the front word);
//   frame_shift, BandBest and band_publish are there too, shared with the other banded kernels.
#include "sa_band_pipe.hpp"

namespace sa {

template <int CPL, int SUBST, bool GENERAL, bool FILL, bool SW>
__global__ void __launch_bounds__(kWave)
band_strips_kernel(const SaBandWideParams<SaBandSwParams> wp) {
  const SaBandSwParams &kp = wp.s;
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
  const Border bd{p.floor, p.gap_open, p.ext, SW, (p.flags & SA_F_NO_START_GAP) != 0};

  // my rows, and whether my neighbours have any
  const long long cend = min((long long)la, c0 + F);
  const long long jf = max(1ll, c0 + 1 - d_hi), jl = la ? min((long long)lb, cend - d_lo) : 0;
  const bool has_rows = jf <= jl;
  const long long jl_left = min((long long)lb, c0 - d_lo);   // the left strip's last row
  const bool left_rows = strip > 0 && jl_left >= 1;
  const bool right_rows = lb >= 1 && c0 + F < (long long)la && c0 + F + 1 <= (long long)lb + d_hi;

  const uint64_t hbase = wp.w.hand_off[pair];
  int2 *hand_out = reinterpret_cast<int2 *>(wp.w.handoff) + hbase + (uint64_t)strip * (uint32_t)width;
  const int2 *hand_in = reinterpret_cast<const int2 *>(wp.w.handoff) + hbase + (uint64_t)(strip ? strip - 1 : 0) * (uint32_t)width;

  int32_t *Mg = nullptr, *Ag = nullptr, *Bg = nullptr;   // cell (i, j) at [j (width - 1) + i]
  if constexpr (FILL && SW) {
    const long long first = d_hi < 0 ? 1 - (long long)d_hi : 1;   // sa_band_sw_rows' j0: the first row stored
    const long long mo = (long long)p.mat_off[pair] - d_lo - first * width;
    Mg = p.M + mo; Ag = p.A + mo; Bg = p.B + mo;
  }
  if constexpr (FILL && !SW) {
    const uint64_t mo = p.mat_off[pair];
    Mg = p.M + mo - d_lo; Ag = p.A + mo - d_lo; Bg = p.B + mo - d_lo;
    if (strip == 0) {   // the band's border cells (reference alignment.c:46-81): strip 0 writes them all
      const uint32_t top = min(la, (uint32_t)d_hi), left = min(lb, (uint32_t)(-d_lo));
      for (uint32_t i = lane; i <= top; i += kWave) {
        const int fl = (i == 0) ? 0 : k.floor_;
        Mg[i] = fl;
        Ag[i] = fl;
        Bg[i] = (i == 0) ? 0 : bd.edge_gap(i);
      }
      for (uint32_t j = 1 + lane; j <= left; j += kWave) {
        const uint64_t c = (uint64_t)j * (uint32_t)(width - 1);
        Mg[c] = k.floor_;
        Ag[c] = bd.edge_gap(j);
        Bg[c] = k.floor_;
      }
    }
  }

  if constexpr (SW) {
    if (!has_rows) {
      // no band cell in my columns.  A pair without any inner band cell gets its (empty) result from strip 0
      const long long colmin = max(1ll, 1ll + d_lo), colmax = min((long long)la, (long long)lb + d_hi);
      if (strip == 0 && (la == 0 || lb == 0 || colmin > colmax) && lane == 0) {
        bp.score[pair] = 0; kp.end_a[pair] = 0; kp.end_b[pair] = 0;
      }
      band_publish(word, front, kAllRows);
      return;
    }
  }

  RowSweep<CPL, SUBST, GENERAL> sw;
  const int g0 = lane * CPL;   // my first frame position
  // the frame of the row before my first: on column max(c0 + 1, d_lo) (d_lo > c0 + 1 only in SW, and then jf = 1)
  const int fc_before = (int)max(c0 + 1, (long long)d_lo);
  sw.start_strip(p, k, bd, sa_, la, (uint32_t)c0, (uint32_t)(fc_before - 1 + g0), lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  if (jf > 1) {   // the row above my first is outside the band in all my columns
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      sw.X[c] = k.floor_;
      sw.Ap[c] = k.floor_;
      if constexpr (GENERAL) sw.Y[c] = k.floor_;
    }
  }
  BandBest<SW ? CPL : 1> best;
  if constexpr (SW) best.init();

  bool left_done = !left_rows;
  int code_b = 0, fz = 0, fb = 0;   // lane t: row j0 + t's code and the feed from the left
  int oz = 0, ob = 0;               // lane t: row j0 + t's values of my last column
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
      fz = fb = k.floor_;
      if ((long long)r <= jl) {
        code_b = p.code[sb_[r - 1]];
        if (strip == 0) {   // the border column while it is in the band (reference alignment.c:72-80)
          if ((long long)r <= -(long long)d_lo) fz = max(k.floor_, bd.edge_gap(r));
        } else {
          const long long e = (long long)r - e_in0;
          if (e >= 0 && e < width) { const int2 h = hand_in[e]; fz = h.x; fb = h.y; }
        }
      }
      if (j == (uint32_t)jf && jf > 1) {   // the up-left of my first row: (c0, jf - 1), on the band's right edge
        if (strip == 0) sw.boundX = k.floor_;
        else { const int2 h = hand_in[0]; sw.boundX = max(h.x, h.y); }
      }
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const long long jd = (long long)j + d_lo;
    const int fc = (int)max(c0 + 1, jd);
    if (jd >= c0 + 2) {   // the frame moves (wave-uniform)
      sw.boundX = read_lane(sw.X[0], 0);
      frame_shift(sw.X, k.floor_);
      frame_shift(sw.Ap, k.floor_);
      if constexpr (GENERAL) frame_shift(sw.Y, k.floor_);
      frame_shift(sw.fa, 0);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, 0);
      if constexpr (SW) best.retire(fc - 1);
    }
    // the cell above the band's right edge is outside the band: the floor
    const long long jh = (long long)j + d_hi;
    const int ge = (int)min(jh - fc, (long long)F) - g0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? k.floor_ : sw.X[c];
      sw.Ap[c] = edge ? k.floor_ : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? k.floor_ : sw.Y[c];
    }
    const int n_row = (int)(min(cend, jh) - fc + 1);   // my band columns of the row
    const int ncol = max(0, min(CPL, n_row - g0));
    const uint32_t col0 = (uint32_t)(fc - 1 + g0);
    int mv[CPL], av[CPL], bv[CPL];
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), read_lane(fz, q), read_lane(fb, q), mv, av, bv);
    if constexpr (SW) best.row(mv, j, ncol);
    if constexpr (FILL) {
      const uint64_t off = (uint64_t)j * (uint32_t)(width - 1) + col0 + 1;
      if (ncol == CPL) {
        store_run<CPL, true>(Mg + off, mv);
        store_run<CPL, true>(Ag + off, av);
        store_run<CPL, true>(Bg + off, bv);
      } else if (ncol > 0) {
        store_partial<CPL>(Mg + off, mv, ncol);
        store_partial<CPL>(Ag + off, av, ncol);
        store_partial<CPL>(Bg + off, bv, ncol);
      }
    }
    if (right_rows) {   // my last column, c0 + F (<= len_a here), at frame position c0 + F - fc
      const int pl = (int)(c0 + F - fc);
      const int cc = pl % CPL;
      int zs = k.floor_, bs = k.floor_;
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (c == cc) { zs = max(mv[c], av[c]); bs = bv[c]; }
      const bool inb = jh >= c0 + F;   // (its lower edge j + d_lo <= c0 + F holds on all my rows)
      const int z = inb ? read_lane(zs, pl / CPL) : k.floor_, b = inb ? read_lane(bs, pl / CPL) : k.floor_;
      oz = (lane == q) ? z : oz;
      ob = (lane == q) ? b : ob;
      if (q == kWave - 1 || j == (uint32_t)jl) {
        const long long e = (long long)j - q + lane - e_out0;
        if (lane <= q && e >= 0 && e < width) hand_out[e] = make_int2(oz, ob);
        if (j != (uint32_t)jl) band_publish(word, front, j);   // (the last rows are published below, after the best cell)
      }
    }
  }

  const unsigned long long err = sw.reduce_err();
  if (lane == 0 && err != ~0ull) {
    atomicMin(reinterpret_cast<unsigned long long *>(p.status + pair), err);
    atomicOr(bp.err_flag, 1u);
  }
  if constexpr (SW) {
    int score;
    unsigned long long key;
    best.reduce((int)max(c0 + 1, jl + d_lo) + g0, score, key);   // the last row's frame
    const uint64_t slot = wp.w.slot_off[pair] + strip;
    if (left_rows) {   // the best of the strips to my left: written before that strip's last publication
      if (!band_strip_wait(word - 1, front, kAllRows)) {
        band_give_up(wp.w.give_up, pair, word, front);
        return;
      }
      merge_left_best(wp.w.strip_best + 4 * (slot - 1), score, key);
    }
    const uint32_t ea = score > 0 ? (uint32_t)(key >> 32) : 0u, eb = score > 0 ? (uint32_t)key : 0u;
    if (lane == 0) {
      if (!right_rows) {
        bp.score[pair] = score; kp.end_a[pair] = ea; kp.end_b[pair] = eb;
      } else {
        *reinterpret_cast<uint4 *>(wp.w.strip_best + 4 * slot) = make_uint4((uint32_t)score, ea, eb, 0u);
      }
    }
  }
  if constexpr (!FILL && !SW) {
    if (la == 0) {   // cell (0, len_b) of the border column
      if (lane == 0) bp.score[pair] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
    } else if (c0 + F >= (long long)la) {   // the last strip: column len_a in the last row's frame
      const int at = (int)((long long)la - max(c0 + 1, (long long)lb + d_lo)) - g0;
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (c == at) bp.score[pair] = sw.X[c];   // max(M, A, B) of (len_a, len_b)
    }
  }
  band_publish(word, front, kAllRows);
}

template <bool FILL, bool SW>
static hipError_t launch_band_strips(const SaBandWideParams<SaBandSwParams> &p, uint32_t strip_cols, const dim3 grid, hipStream_t stream) {
  return launch_by_strip_cols(strip_cols, [&](auto cpl) {
    launch_by_scoring(p.s.b.f, [&](auto subst, auto general, uint32_t table_ints) {
      hipLaunchKernelGGL((band_strips_kernel<cpl(), subst(), general(), FILL, SW>), grid, dim3(kWave), table_ints * sizeof(int32_t), stream, p);
    });
    return hipGetLastError();
  });
}

}  // namespace sa

hipError_t sa_launch_band_strips(const SaBandWideParams<SaBandSwParams> &p, uint32_t strip_cols, bool fill, bool is_sw, uint64_t items, hipStream_t stream) {
  if (p.s.b.f.n_pairs == 0) return hipSuccess;
  dim3 grid;
  if (sa::band_strips_grid(p.s.b.f.n_pairs, p.w.strips_per_pair, grid) != hipSuccess) return hipErrorInvalidValue;
  sa_record_launch_ext(fill ? SEQALIGN_KX_BAND_FILL : SEQALIGN_KX_BAND_SCORE, items);
  if (is_sw) return fill ? sa::launch_band_strips<true, true>(p, strip_cols, grid, stream) : sa::launch_band_strips<false, true>(p, strip_cols, grid, stream);
  return fill ? sa::launch_band_strips<true, false>(p, strip_cols, grid, stream) : sa::launch_band_strips<false, false>(p, strip_cols, grid, stream);
}
