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
#pragma once
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
      span_frame_shift(sw.X, 0);
      span_frame_shift(sw.Ap, 0);
      if constexpr (GENERAL) span_frame_shift(sw.Y, 0);
      span_frame_shift(sw.fa, cin & 0xff);
      if constexpr (SUBST != SA_SUBST_SIMPLE) span_frame_shift(sw.arow, (cin >> 8) * k.K);
      span_frame_shift(P::D0(sw), 0u); span_frame_shift(P::D1(sw), 0u);
      span_frame_shift(P::V0(sw), 0u); span_frame_shift(P::V1(sw), 0u);
      // column fc - 1 leaves through lane 0
      const int s0 = read_lane(sw.bs[0], 0);
      if (s0 > ret_s) {
        ret_s = s0; ret_col = (uint32_t)(fc - 1);
        ret_row = (uint32_t)read_lane((int)sw.br[0], 0);
        ret_0 = (uint32_t)read_lane((int)P::best0(sw)[0], 0);
        ret_1 = (uint32_t)read_lane((int)P::best1(sw)[0], 0);
      }
      span_frame_shift(sw.bs, 0);
      span_frame_shift(sw.br, 0u); span_frame_shift(P::best0(sw), 0u); span_frame_shift(P::best1(sw), 0u);
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

}  // namespace sa
