// sa_band.hip -- banded NW: the row sweep of every fill (sa_rowsweep.hpp) in a frame that follows a diagonal band down the
// matrix, and the walk over what it stored.  The contract (include/seqalign_hip.h): pair k has the band
//     d_lo <= i - j <= d_hi = d_lo + width - 1          (i: column of seq_a, j: row of seq_b; d_lo <= 0 <= d_hi)
// and the banded matrices are the reference's recurrence (src/alignment.c:28-168) with every cell outside the band, border
// cells too, at the floor in all three matrices.
//
// band_rows_kernel: one wave per pair, a frame of F = 64 x CPL cells, CPL from the ladder by the pair's width (F >= width).
//   Frame.  On row j the frame's first column is fc(j) = max(1, j + d_lo); position g = lane * CPL + c of the frame is column
//   fc(j) + g.  Rows j <= -d_lo: the border column is in the band and is the feed, as in score_rows_kernel.  From row
//   -d_lo + 1 on the cell left of the frame is outside the band: the feed is the floor.  From row -d_lo + 2 on fc moves one
//   column per row: before row j the previous row (X, Ap, Y) and the columns' codes (fa, arow) shift left by one position --
//   registers within a lane, one wave_shl:1 DPP per array across lanes -- boundX (the up-left of position 0) becomes lane 0's
//   X[0] from before the shift (the cell (fc(j) - 1, j - 1), in the band: same diagonal as (fc(j), j)), and the position that
//   enters on the right gets its seq_a code (fetched 64 rows at a time, like seq_b's) and the floor.  RowSweep's gap_b scan
//   constants c1 / c2 / c3 are in frame positions and stay.
//   Band edges are exact.  Which cells can a band cell (i, j) read?  (i - 1, j - 1): its own diagonal, in the band.
//   (i - 1, j): the gap_b scan runs left to right, so nothing right of a cell reaches it; left of the band's first cell is the
//   feed (above).  (i, j - 1): diagonal i - j + 1, outside the band exactly when (i, j) is on the right edge i - j = d_hi.
//   So before row j the ONE position that holds column j + d_hi -- g_e = j + d_hi - fc(j): d_hi - d_lo while the frame moves,
//   j + d_hi - 1 before; always < width <= F -- gets the floor in X, Ap and Y, whatever the sweep computed there on row
//   j - 1 (on row 0: the border value of (d_hi + 1, 0), outside the band).  That holds in both phases and when F > width.
//   Positions right of that, and columns right of len_a, hold whatever the sweep makes of them: no band cell reads them (they
//   are to the right on the same row, or above cells that are themselves outside), ncol (the lane's count of band columns
//   <= len_a on this row) keeps them out of the error key and out of the stores, and every add is addw.
//   Score form: nothing stored per cell; after the last row X of column len_a is max(M, A, B) of (len_a, len_b), the
//   reference's end pick (needleman_wunsch.c:54-66), as in score_rows_kernel.
//   Fill form: M, A, B of the band's cells, row j holding diagonals d_lo .. d_hi: cell (i, j) at j (width - 1) + i - d_lo,
//   64-bit.  The band's border cells (row 0: columns 0 .. d_hi; column 0: rows 1 .. -d_lo) are written up front.
//
// band_walk_kernel: traceback_kernel's end pick, walk and leading gaps, one lane per pair, all pairs of a chunk in one
//   launch.  reverse_move_t reads through BandAccess: a cell outside the band is the floor in all three matrices, as the
//   contract says, so a walk that the floor's arithmetic lets out of the band (free end gaps: floor + 0 == floor) goes on
//   exactly as the reference's would over the banded matrices.
//
// Banded SW (seqalign_sw_*_banded) is the same sweep, band_rows_kernel<.., SW = true> on SaBandSwParams, and a walk of its own
// (band_sw_walk_kernel).  The band is the caller's -- any d_lo <= d_hi inside [-len_b, len_a] -- and every cell outside it,
// like every border cell, holds 0 in all three matrices.  What differs from NW:
//   Frame.  fc(j) = max(1, j + d_lo) as above, for any sign of d_lo: with d_lo >= 1 the frame moves from row 1 on, so row 0's
//   frame starts at column d_lo; with d_hi < 0 the first row that has a band cell is 1 - d_hi and the sweep starts there, on
//   the all-zero state (the frame still stands at column 1 then: d_lo <= d_hi < 0).  The last row swept is
//   min(len_b, len_a - d_lo), the last that has one (sa_band_sw_rows).  Feed, entering positions and the cell above the
//   right edge are the floor as in NW -- the SW floor, 0.
//   Best cell.  BandBest keeps, per frame POSITION, the best match_scores value of the column that position holds and the
//   first row that reached it; when the frame moves, the column that leaves through lane 0 is merged into a wave-uniform
//   "retired" best (strict >: retired columns are lower than it, and they keep a tie) and the per-position bests shift with
//   the frame.  The end pick is the retired best, then the live columns ascending: score desc, column asc, row asc.
//   Fill form: M, A, B of rows j0 .. j1 only, row j holding diagonals d_lo .. d_hi: cell (i, j) at (j - j0) width + i - j -
//   d_lo; no border cell is stored (BandSwAccess reads them, like the cells outside the band, as 0).  It reports the best
//   cell itself, as the score form does.
//   Walk: traceback_kernel's SW walk from the best cell until the score is 0, pos / len / length as it reports them.
#include "sa_band_pipe.hpp"   // wave_shl1, frame_shift, BandBest
#include "sa_trace_common.hpp"

namespace sa {

__host__ __device__ __forceinline__ const SaBandParams &band_params(const SaBandParams &p) { return p; }
__host__ __device__ __forceinline__ const SaBandParams &band_params(const SaBandSwParams &p) { return p.b; }

// The sweep of both band families.  SW = false: banded NW.  SW = true: banded SW (header).
template <int CPL, int SUBST, bool GENERAL, bool FILL, bool SW = false>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
band_rows_kernel(const std::conditional_t<SW, SaBandSwParams, SaBandParams> kp) {
  const SaBandParams &bp = band_params(kp);
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
  const Border bd{p.floor, p.gap_open, p.ext, SW, (p.flags & SA_F_NO_START_GAP) != 0};

  // SW: the first row that has a band cell
  const uint32_t first = (SW && d_hi < 0) ? (uint32_t)(1 - d_hi) : 1u;

  int32_t *Mg = nullptr, *Ag = nullptr, *Bg = nullptr;   // cell (i, j) at [j (width - 1) + i]
  if constexpr (FILL && SW) {
    const long long mo = (long long)p.mat_off[pair] - d_lo - (long long)first * width;   // row `first` is the first stored
    Mg = p.M + mo; Ag = p.A + mo; Bg = p.B + mo;
  }
  if constexpr (FILL && !SW) {
    const uint64_t mo = p.mat_off[pair];
    Mg = p.M + mo - d_lo; Ag = p.A + mo - d_lo; Bg = p.B + mo - d_lo;
    // the band's border cells (reference alignment.c:46-81)
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

  RowSweep<CPL, SUBST, GENERAL> sw;
  const int g0 = lane * CPL;   // my first frame position
  // SW: the frame of the row before the first stands at column max(1, d_lo), over zeros
  sw.start_strip(p, k, bd, sa_, la, 0, (uint32_t)(SW ? max(1, d_lo) - 1 + g0 : g0), lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  BandBest<SW ? CPL : 1> best;
  if constexpr (SW) best.init();

  // len_a == 0: the border column is the whole matrix.  SW: rows past the band's last cell are not swept
  const uint32_t rows = la ? (SW ? min(lb, (uint32_t)((int)la - d_lo)) : lb) : 0;
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
    if (jd >= 2) {   // the frame moves (wave-uniform)
      const int cin = read_lane(code_in, q);
      sw.boundX = read_lane(sw.X[0], 0);
      frame_shift(sw.X, k.floor_);
      frame_shift(sw.Ap, k.floor_);
      if constexpr (GENERAL) frame_shift(sw.Y, k.floor_);
      frame_shift(sw.fa, cin & 0xff);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, (cin >> 8) * k.K);
      if constexpr (SW) best.retire(fc - 1);
    }
    // the cell above the band's right edge is outside the band: the floor (header)
    const int ge = (int)j + d_hi - fc - g0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? k.floor_ : sw.X[c];
      sw.Ap[c] = edge ? k.floor_ : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? k.floor_ : sw.Y[c];
    }
    const int n_row = min((int)la, (int)j + d_hi) - fc + 1;   // band columns of the row in the frame
    const int ncol = max(0, min(CPL, n_row - g0));
    const uint32_t col0 = (uint32_t)(fc - 1 + g0);
    // the cell left of the frame: the border column while it is in the band, else the floor
    const int feedZ = (jd <= 0) ? max(k.floor_, bd.edge_gap(j)) : k.floor_, feedB = k.floor_;
    int mv[CPL], av[CPL], bv[CPL];
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), feedZ, feedB, mv, av, bv);
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
  }

  const unsigned long long err = sw.reduce_err();
  if constexpr (SW) {
    int score;
    unsigned long long key;
    best.reduce(max(1, (int)rows + d_lo) + g0, score, key);   // the last row's frame (no row swept: every best is 0)
    if (lane == 0) {
      bp.score[pair] = score;
      kp.end_a[pair] = score > 0 ? (uint32_t)(key >> 32) : 0u;
      kp.end_b[pair] = score > 0 ? (uint32_t)key : 0u;
    }
  }
  if constexpr (!FILL && !SW) {
    if (la == 0) {   // cell (0, len_b) of the border column
      if (lane == 0) bp.score[pair] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
    } else {
      const int at = (int)la - max(1, (int)lb + d_lo) - g0;   // column len_a in the last row's frame
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (c == at) bp.score[pair] = sw.X[c];   // max(M, A, B) of (len_a, len_b)
    }
  }
  if (lane == 0) {
    p.status[pair] = err;
    if (err != ~0ull) atomicOr(bp.err_flag, 1u);
  }
}

// reverse_move_t's view of a band: a cell outside it is the floor
struct BandAccess {
  const uint8_t *seq_a, *seq_b;
  const uint16_t *code;
  const int32_t *M, *A, *B;   // cell (x, y) at [y pitch + x]
  uint64_t pitch;             // width - 1
  long long d_lo, d_hi;
  int floor_;
  __device__ __forceinline__ int code_a(uint32_t i) const { return code[seq_a[i]]; }
  __device__ __forceinline__ int code_b(uint32_t j) const { return code[seq_b[j]]; }
  __device__ __forceinline__ void cell(uint32_t x, uint32_t y, int &m, int &a, int &b) const {
    const long long d = (long long)x - (long long)y;
    m = a = b = floor_;
    if (d >= d_lo && d <= d_hi) {
      const uint64_t at = (uint64_t)y * pitch + x;
      m = M[at]; a = A[at]; b = B[at];
    }
  }
};

__global__ void __launch_bounds__(kWave) band_walk_kernel(const SaBandParams bp) {
  const SaFillParams &p = bp.f;
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= p.n_pairs) return;
  const uint32_t la = p.len_a[w], lb = p.len_b[w];
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[w];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[w];
  const int d_lo = bp.d_lo[w];
  const uint32_t width = bp.width[w];
  const uint64_t mo = p.mat_off[w];
  const BandAccess acc{sa_, sb_, p.code, p.M + mo - d_lo, p.A + mo - d_lo, p.B + mo - d_lo, (uint64_t)(width - 1),
                       (long long)d_lo, (long long)d_lo + width - 1, p.floor};
  const TraceConsts k{p.code, p.table, (int)p.K, p.open1, p.ext, p.gen_eq, p.gen_ne,
                      (p.flags & SA_F_NO_START_GAP) != 0, (p.flags & SA_F_NO_END_GAP) != 0,
                      (p.flags & SA_F_NO_GAPS_A) != 0, (p.flags & SA_F_NO_GAPS_B) != 0};
  char *oa = bp.out_a + bp.str_off[w];
  char *ob = bp.out_b + bp.str_off[w];

  // end cell: ties resolve GAP_A > GAP_B > MATCH (needleman_wunsch.c:53-66)
  uint32_t x = la, y = lb, head = la + lb, err = 0;
  int matrix = MAT_MATCH, score, a0, b0;
  acc.cell(x, y, score, a0, b0);
  if (b0 >= score) { matrix = MAT_GAP_B; score = b0; }
  if (a0 >= score) { matrix = MAT_GAP_A; score = a0; }
  const int end_score = score;

  while (x > 0 && y > 0) {
    if (head == 0) { err = SEQALIGN_E_TRACEBACK; break; }   // (cannot happen: every step lowers x or y)
    --head;
    oa[head] = (matrix == MAT_GAP_A) ? '-' : (char)sa_[x - 1];
    ob[head] = (matrix == MAT_GAP_B) ? '-' : (char)sb_[y - 1];
    if ((err = reverse_move_t(acc, k, la, lb, x, y, matrix, score))) break;
  }
  if (!err) {
    for (; y > 0; --y) { --head; oa[head] = '-'; ob[head] = (char)sb_[y - 1]; }   // needleman_wunsch.c:117-123
    for (; x > 0; --x) { --head; oa[head] = (char)sa_[x - 1]; ob[head] = '-'; }   // :126-132
  }
  // SEQALIGN_E_UNKNOWN_PAIR first: the fill met a band cell without a score and left the floor in it, so a walk that fails
  // may have failed for that; the pair's answer does not depend on where the cell lies
  if (p.status[w] != ~0ull) err = SEQALIGN_E_UNKNOWN_PAIR;
  *reinterpret_cast<uint4 *>(bp.meta4 + 4ull * w) = make_uint4(head, la + lb - head, (uint32_t)end_score, err);
}

// banded SW: border cells and cells outside the band are 0; band cell (x, y) of rows j0 .. at [(y - j0) width + x - y - d_lo]
struct BandSwAccess {
  const uint8_t *seq_a, *seq_b;
  const uint16_t *code;
  const int32_t *M, *A, *B;   // cell (x, y) at [y pitch + x]
  uint64_t pitch;             // width - 1
  long long d_lo, d_hi;
  __device__ __forceinline__ int code_a(uint32_t i) const { return code[seq_a[i]]; }
  __device__ __forceinline__ int code_b(uint32_t j) const { return code[seq_b[j]]; }
  __device__ __forceinline__ void cell(uint32_t x, uint32_t y, int &m, int &a, int &b) const {
    const long long d = (long long)x - (long long)y;
    m = a = b = 0;
    if (x > 0 && y > 0 && d >= d_lo && d <= d_hi) {
      const uint64_t at = (uint64_t)y * pitch + x;
      m = M[at]; a = A[at]; b = B[at];
    }
  }
};

// traceback_kernel's SW walk from the best cell the fill form reported, one lane per pair.  meta8[8w..]: score, status, pos_a,
// pos_b, end_a, end_b, length, head (the strings: [head, len_a + len_b) of the pair's slot).  Score 0: no walk, length 0.
__global__ void __launch_bounds__(kWave) band_sw_walk_kernel(const SaBandSwParams sp) {
  const SaBandParams &bp = sp.b;
  const SaFillParams &p = bp.f;
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= p.n_pairs) return;
  const uint32_t la = p.len_a[w], lb = p.len_b[w];
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[w];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[w];
  const int d_lo = bp.d_lo[w];
  const uint32_t width = bp.width[w];
  const long long d_hi = (long long)d_lo + width - 1;
  const long long first = d_hi < 0 ? 1 - d_hi : 1;
  const long long mo = (long long)p.mat_off[w] - d_lo - first * width;
  const BandSwAccess acc{sa_, sb_, p.code, p.M + mo, p.A + mo, p.B + mo, (uint64_t)(width - 1), (long long)d_lo, d_hi};
  const TraceConsts k{p.code, p.table, (int)p.K, p.open1, p.ext, p.gen_eq, p.gen_ne,
                      (p.flags & SA_F_NO_START_GAP) != 0, (p.flags & SA_F_NO_END_GAP) != 0,
                      (p.flags & SA_F_NO_GAPS_A) != 0, (p.flags & SA_F_NO_GAPS_B) != 0};
  char *oa = bp.out_a + bp.str_off[w];
  char *ob = bp.out_b + bp.str_off[w];

  const int end_score = bp.score[w];
  const uint32_t end_x = sp.end_a[w], end_y = sp.end_b[w];
  uint32_t x = end_x, y = end_y, head = la + lb, err = 0;
  int matrix = MAT_MATCH, score = end_score;
  // SEQALIGN_E_UNKNOWN_PAIR first, as band_walk_kernel: the pair's answer does not depend on where the cell lies
  if (p.status[w] != ~0ull) err = SEQALIGN_E_UNKNOWN_PAIR;
  while (!err && score > 0) {
    if (head == 0) { err = SEQALIGN_E_TRACEBACK; break; }   // (cannot happen: every step lowers x or y)
    --head;
    oa[head] = (matrix == MAT_GAP_A) ? '-' : (char)sa_[x - 1];
    ob[head] = (matrix == MAT_GAP_B) ? '-' : (char)sb_[y - 1];
    err = reverse_move_t(acc, k, la, lb, x, y, matrix, score);
  }
  uint4 *out = reinterpret_cast<uint4 *>(sp.meta8 + 8ull * w);
  out[0] = make_uint4((uint32_t)end_score, err, x, y);   // smith_waterman.c:249-255
  out[1] = make_uint4(end_x, end_y, la + lb - head, head);
}

template <int CPL, bool FILL, bool SW, class P>
static hipError_t launch_band_cpl(const P &p, hipStream_t stream) {
  const SaFillParams &f = band_params(p).f;
  const dim3 grid((f.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((band_rows_kernel<CPL, subst(), general(), FILL, SW>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

// the columns per lane of the widest band (sa_score_row_class's steps)
template <bool FILL, bool SW = false, class P>
static hipError_t launch_band(const P &p, uint32_t max_width, hipStream_t stream) {
  const uint32_t need = columns_per_lane(max_width);
  return launch_by_cpl<1, 2, 3, 4, 5, 6, 8, 12, 16>(need, [&](auto cpl) { return launch_band_cpl<cpl(), FILL, SW>(p, stream); });
}

}  // namespace sa

hipError_t sa_launch_band_score(const SaBandParams &p, uint32_t max_width, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, p.f.n_pairs);
  return sa::launch_band<false>(p, max_width, stream);
}

hipError_t sa_launch_band_fill(const SaBandParams &p, uint32_t max_width, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_FILL, p.f.n_pairs);
  return sa::launch_band<true>(p, max_width, stream);
}

hipError_t sa_launch_band_walk(const SaBandParams &p, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  sa_record_launch_ext(SEQALIGN_KX_BAND_WALK, p.f.n_pairs);
  hipLaunchKernelGGL(sa::band_walk_kernel, dim3((p.f.n_pairs + sa::kWave - 1) / sa::kWave), dim3(sa::kWave), 0, stream, p);
  return hipGetLastError();
}

// banded SW: counted under the same three kinds (include/seqalign_hip.h: the second launch record is pinned)
hipError_t sa_launch_band_sw_score(const SaBandSwParams &p, uint32_t max_width, hipStream_t stream) {
  if (p.b.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, p.b.f.n_pairs);
  return sa::launch_band<false, true>(p, max_width, stream);
}

hipError_t sa_launch_band_sw_fill(const SaBandSwParams &p, uint32_t max_width, hipStream_t stream) {
  if (p.b.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_FILL, p.b.f.n_pairs);
  return sa::launch_band<true, true>(p, max_width, stream);
}

hipError_t sa_launch_band_sw_walk(const SaBandSwParams &p, hipStream_t stream) {
  if (p.b.f.n_pairs == 0) return hipSuccess;
  sa_record_launch_ext(SEQALIGN_KX_BAND_WALK, p.b.f.n_pairs);
  hipLaunchKernelGGL(sa::band_sw_walk_kernel, dim3((p.b.f.n_pairs + sa::kWave - 1) / sa::kWave), dim3(sa::kWave), 0, stream, p);
  return hipGetLastError();
}
