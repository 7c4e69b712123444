// sa_band_span.hip -- banded SW hit spans (seqalign_sw_span_banded): score, start and end of the best local hit inside a band
// of diagonals, nothing stored per cell, no walk.  band_rows_kernel<.., FILL = false, SW = true>'s frame (sa_band.hip: the
// frame, its shift, the floor above the right edge, the rows swept) around SpanSweep's arithmetic (sa_span.hpp; the
// definition of a span and the tie argument: sa_span.hip's header).  The definition carries over with one
// rule more: a cell outside the band is a stop -- it holds 0 in all three states and its span is the cell itself (3.19).
//
// band_span_rows_kernel: one wave per pair, 4 pairs per workgroup, a frame of F = 64 x CPL positions, CPL from {1 .. 6, 8} by
// the launch's widest band.  Position g = lane * CPL + c holds column fc(j) + g on row j, fc(j) = max(1, j + d_lo).  What the
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
#include "sa_span.hpp"

namespace sa {

// wave_shl:1, the mirror of wave_shr1 (as sa_band.hip): lane l receives src of lane l + 1, lane 63 lane63_value
__device__ __forceinline__ int band_span_shl1(int src, int lane63_value) {
  return __builtin_amdgcn_update_dpp(lane63_value, src, 0x130, 0xf, 0xf, false);
}

// sa_band.hip's frame_shift for the sweep's int and uint32_t arrays
template <class T, int N>
__device__ __forceinline__ void span_frame_shift(T (&a)[N], T enters) {
  const T first = a[0];
#pragma unroll
  for (int c = 0; c + 1 < N; ++c) a[c] = a[c + 1];
  a[N - 1] = (T)band_span_shl1((int)first, (int)enters);
}

template <int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
band_span_rows_kernel(const SaBandSpanParams kp) {
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
  SpanSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, sa_, la, (uint32_t)(max(1, d_lo) - 1), (uint32_t)(max(1, d_lo) - 1 + g0), lane);
#pragma unroll
  for (int c = 0; c < CPL; ++c) sw.Dy[c] = sw.Vy[c] = first - 1;   // the zeros of row first - 1 are stops of their own (rule 2)
  sw.boundDy = first - 1;
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  // of the columns left of the frame (wave-uniform): best value, its column and first row, that cell's span
  int ret_s = 0;
  uint32_t ret_col = 0, ret_row = 0, ret_x = 0, ret_y = 0;

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
      sw.boundDx = (uint32_t)read_lane((int)sw.Dx[0], 0);
      sw.boundDy = (uint32_t)read_lane((int)sw.Dy[0], 0);
      span_frame_shift(sw.X, 0);
      span_frame_shift(sw.Ap, 0);
      if constexpr (GENERAL) span_frame_shift(sw.Y, 0);
      span_frame_shift(sw.fa, cin & 0xff);
      if constexpr (SUBST != SA_SUBST_SIMPLE) span_frame_shift(sw.arow, (cin >> 8) * k.K);
      span_frame_shift(sw.Dx, 0u); span_frame_shift(sw.Dy, 0u);
      span_frame_shift(sw.Vx, 0u); span_frame_shift(sw.Vy, 0u);
      // column fc - 1 leaves through lane 0
      const int s0 = read_lane(sw.bs[0], 0);
      if (s0 > ret_s) {
        ret_s = s0; ret_col = (uint32_t)(fc - 1);
        ret_row = (uint32_t)read_lane((int)sw.br[0], 0);
        ret_x = (uint32_t)read_lane((int)sw.bx[0], 0);
        ret_y = (uint32_t)read_lane((int)sw.by[0], 0);
      }
      span_frame_shift(sw.bs, 0);
      span_frame_shift(sw.br, 0u); span_frame_shift(sw.bx, 0u); span_frame_shift(sw.by, 0u);
    }
    // the cell above the band's right edge is outside the band: 0, and a stop of its own (rule 2)
    const int ge = (int)j + d_hi - fc - g0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? 0 : sw.X[c];
      sw.Ap[c] = edge ? 0 : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? 0 : sw.Y[c];
      sw.Vx[c] = edge ? (uint32_t)((int)j + d_hi) : sw.Vx[c];
      sw.Vy[c] = edge ? j - 1 : sw.Vy[c];
    }
    const int n_row = min((int)la, (int)j + d_hi) - fc + 1;   // band columns of the row in the frame
    const int ncol = max(0, min(CPL, n_row - g0));
    const uint32_t col0 = (uint32_t)(fc - 1 + g0);
    // the cell left of the frame: the border column or a cell outside the band, 0 and its own span either way
    const SpanFeed f{0, 0, 0, (uint32_t)(fc - 1), j, (uint32_t)(fc - 1), j};
    SpanFeed out;
    sw.template row<true>(k, j, lb, la, W, lane, col0, ncol, read_lane(code_b, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  int score;
  unsigned long long key, span;
  // the last row's frame (no row swept: every best is 0); a position that never held a band column has kept 0
  sw.reduce_best((uint32_t)(max(1, (int)rows + d_lo) - 1 + g0), CPL, score, key, span);
  if (ret_s >= score && ret_s > 0) {   // a tie goes to the lower column: a retired one
    score = ret_s;
    key = ((unsigned long long)ret_col << 32) | ret_row;
    span = ((unsigned long long)ret_x << 32) | ret_y;
  }
  if (lane == 0) {
    const bool hit = score > 0;
    const uint32_t ea = hit ? (uint32_t)(key >> 32) : 0u, eb = hit ? (uint32_t)key : 0u;
    const uint32_t pa = hit ? (uint32_t)(span >> 32) : 0u, pb = hit ? (uint32_t)span : 0u;
    bp.score[pair] = hit ? score : 0;
    kp.pos_a[pair] = pa; kp.pos_b[pair] = pb;
    kp.len_a[pair] = ea - pa; kp.len_b[pair] = eb - pb;
    p.status[pair] = err;
    if (err != ~0ull) atomicOr(bp.err_flag, 1u);
  }
}

template <int CPL>
static hipError_t launch_band_span_cpl(const SaBandSpanParams &p, hipStream_t stream) {
  const SaFillParams &f = p.b.f;
  const dim3 grid((f.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((band_span_rows_kernel<CPL, subst(), general()>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

hipError_t sa_launch_band_span(const SaBandSpanParams &p, uint32_t max_width, hipStream_t stream) {
  if (p.b.f.n_pairs == 0) return hipSuccess;
  if (max_width == 0 || max_width > SA_SPAN_BAND_MAX_WIDTH) return hipErrorInvalidValue;
  sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, p.b.f.n_pairs);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_width), [&](auto cpl) { return sa::launch_band_span_cpl<cpl()>(p, stream); });
}
