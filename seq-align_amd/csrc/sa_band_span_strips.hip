// sa_band_span_strips.hip -- wide banded SW hit spans (seqalign_sw_span_banded_wide): seqalign_sw_span_banded's five integers at
// any band width and any length, one pair on many waves.  Two things that exist, crossed: the strip pipeline, the moving frame
// and the best cell merged from strip to strip of band_strips_kernel<CPL, SUBST, GENERAL, FILL = false, SW = true>
// (sa_band_strips.hip's header: the strips, their rows, the frame, the hand-off column, the tickets, the bounded wait and the
// give-up word) and the payload rules of the narrow span kernel (sa_band_span.hip's header: the four rules) around
// SpanSweep::row<BAND, PICK>.  It is sa_band_sw_stats_strips.hip's shape with the count-free sweep inside: the two payload words
// are the stop cell's x and y, each a full word, so there is no limit on the lengths.  DESIGN.md 3.28.
//
// band_span_strips_kernel<CPL, SUBST, GENERAL>: one workgroup = one wave = one (pair, strip), drawn by ticket.  Strip s owns
// columns c0 + 1 .. c0 + S, c0 = s S, S = 64 x CPL; its rows jf .. jl, fc(j) = max(c0 + 1, j + d_lo), fc_before = max(c0 + 1,
// d_lo), when the frame moves, ncol, left_rows / right_rows, the early exit of a strip without rows (strip 0 writes the five
// zeros of a pair without inner band cells) and the progress, front and give-up words are band_strips_kernel's, to the letter.
// The payload rules, as they read per strip:
//   Shift (rule 1).  Dx / Dy / Vx / Vy and bs / br / bx / by shift with X, Ap, Y, fa, arow; boundX / boundDx / boundDy become
//     lane 0's [0] from before the shift.  Lane 0's column retires into a wave-uniform best that keeps its span (strict >: a
//     tie stays with the retired, lower column).  What enters on the right is a column past the strip's end, never a cell of
//     this strip: 0 in every word.
//   Outside the band is a stop (rule 2): 0 in all three states, its span the cell itself -- BandSpanFrame::stop0 / stop1, x and
//     y in full words.  That is row jf - 1 in all its columns (row 0 for jf = 1, which start_strip has written so); position
//     g_e = j + d_hi - fc(j), the cell above the band's right edge, where it lies in the frame, in X, Ap, Y, Vx, Vy before every
//     row; the feed left of the frame wherever (c0, j) is no band cell -- on every row once the frame has moved, and strip 0's
//     border column on all its rows -- which is {0, 0, not from A, spans (fc(j) - 1, j)}.
//   Left feed and up-left of a first row.  Strip s > 0, while (c0, j) is a band cell: the left strip's hand-off entry of the
//     row.  The up-left of a first row jf > 1 is (c0, jf - 1), on the band's right edge: hand-off entry 0, merged by row()'s
//     own boundary rule (A >= B > M via from_a).  Strip 0: the border cell (0, jf - 1), a stop of its own.
//   Hand-off.  Per row of the strip's last column c0 + S while that cell is in the band (rows c0 + S - d_hi .. c0 + S - d_lo):
//     StripSpanHandoff's content, 32 bytes at entry [row - (c0 + S - d_hi)] of the strip's `width` entries, moved 64 rows at a
//     time and then published.  The column sits at frame position c0 + S - fc(j), which moves: SpanSweep::row<BAND, PICK>
//     leaves that column's values in `out`, and they are read from the lane that holds it.
//   Best cell.  At the end of a strip reduce_best over the live columns, then the retired best first on a tie; then the wait for
//     the left strip's ~0 and merge_left_best_span (left wins a tie).  A strip with a right neighbour stores {score, end_a,
//     end_b, 0} {pos_a, pos_b, 0, 0} in its 32-byte best entry before its last publication; the last strip of the run unpacks
//     into the five results as BandSpanFrame::write does.
// A frame position right of len_a or of the strip's end holds whatever the sweep computes there; a band cell never reads it
// (sa_band_sw_stats_strips.hip's header gives the argument cell by cell: up-left, above through g_e, the left-to-right scan, the
// feed), it is masked out of the best cell and the error key by ncol, and the hand-off reads column c0 + S only where c0 + S <
// len_a and the cell is in the band.  With full words there is nothing to overflow besides.
// Nothing waits on a strip to its right; every path out of the kernel publishes ~0; no loop is unbounded.
#include "sa_span.hpp"

namespace sa {
namespace wide_span {

constexpr unsigned long long kBandWaitTicks = 200000000ull;   // 2 s of the 100 MHz wall clock
constexpr uint32_t kAllRows = 0xFFFFFFFFu;

// copies of sa_band_strips.hip's helpers (that file's code objects do not change)
__device__ __forceinline__ int wave_shl1(int src, int lane63_value) {
  return __builtin_amdgcn_update_dpp(lane63_value, src, 0x130, 0xf, 0xf, false);   // wave_shl:1
}

template <int N>
__device__ __forceinline__ void frame_shift(int (&a)[N], int enters) {
  const int first = a[0];
#pragma unroll
  for (int c = 0; c + 1 < N; ++c) a[c] = a[c + 1];
  a[N - 1] = wave_shl1(first, enters);
}
template <int N>
__device__ __forceinline__ void frame_shift(uint32_t (&a)[N], uint32_t enters) {
  const uint32_t first = a[0];
#pragma unroll
  for (int c = 0; c + 1 < N; ++c) a[c] = a[c + 1];
  a[N - 1] = (uint32_t)wave_shl1((int)first, (int)enters);
}

__device__ __forceinline__ void band_publish(uint32_t *word, uint32_t *front, uint32_t value) {
  strip_publish(word, value);
  if (threadIdx.x == 0) __hip_atomic_fetch_add(front, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool band_strip_wait(const uint32_t *word, const uint32_t *front, uint32_t need) {
  uint32_t seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  if (seen < need) {
    uint32_t at = __builtin_amdgcn_readfirstlane(__hip_atomic_load(front, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    unsigned long long t0 = wall_clock64();
    for (;;) {
      __builtin_amdgcn_s_sleep(8);
      const uint32_t now = __builtin_amdgcn_readfirstlane(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (now >= need) break;
      const unsigned long long t = wall_clock64();
      if (now != seen) { seen = now; t0 = t; }   // it advanced: the budget restarts
      else if (t - t0 > kBandWaitTicks) {         // has any strip of the pair published since the budget started?
        const uint32_t f = __builtin_amdgcn_readfirstlane(__hip_atomic_load(front, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (f == at) return false;
        at = f; t0 = t;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return true;
}

// the two words of a stop in cell (x, y): BandSpanFrame::stop0 / stop1 (sa_band_span.hip), full words
__device__ __forceinline__ uint32_t stop0(uint32_t x, uint32_t) { return x; }
__device__ __forceinline__ uint32_t stop1(uint32_t, uint32_t y) { return y; }

// BandSpanFrame::write (sa_band_span.hip): the five results from the best cell's key and its span
__device__ __forceinline__ void write_results(const SaBandSpanParams &kp, uint32_t pair, int score, unsigned long long key,
                                              unsigned long long span) {
  const bool hit = score > 0;
  const uint32_t ea = hit ? (uint32_t)(key >> 32) : 0u, eb = hit ? (uint32_t)key : 0u;
  const uint32_t pa = hit ? (uint32_t)(span >> 32) : 0u, pb = hit ? (uint32_t)span : 0u;
  kp.b.score[pair] = hit ? score : 0;
  kp.pos_a[pair] = pa; kp.pos_b[pair] = pb;
  kp.len_a[pair] = ea - pa; kp.len_b[pair] = eb - pb;
}

template <int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
band_span_strips_kernel(const SaBandSpanStripsParams wp) {
  const SaBandSpanParams &kp = wp.s;
  const SaBandParams &bp = kp.b;
  const SaFillParams &p = bp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  constexpr int F = kWave * CPL;   // the strip's columns, and the frame's positions
  const int lane = threadIdx.x;
  uint32_t strip, pair;
  strip_of_ticket(strip_ticket(wp.ticket), wp.strips_per_pair, strip, pair);
  if (pair >= p.n_pairs) return;

  const uint32_t la = p.len_a[pair], lb = p.len_b[pair];
  const long long c0 = (long long)strip * F;
  if (c0 >= (long long)la && strip != 0) return;   // this pair has fewer strips: no progress word, nobody waits for it
  uint32_t *word = wp.progress + wp.slot_off[pair] + strip;
  uint32_t *front = wp.front + pair;   // publications by any strip of the pair

  const int d_lo = __builtin_amdgcn_readfirstlane(bp.d_lo[pair]);
  const int width = __builtin_amdgcn_readfirstlane((int)bp.width[pair]);
  const int d_hi = d_lo + width - 1;
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[pair];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[pair];
  const uint32_t W = la + 1;

  const SweepConsts k(p, table);

  // my rows, and whether my neighbours have any
  const long long cend = min((long long)la, c0 + F);
  const long long jf = max(1ll, c0 + 1 - d_hi), jl = la ? min((long long)lb, cend - d_lo) : 0;
  const bool has_rows = jf <= jl;
  const long long jl_left = min((long long)lb, c0 - d_lo);   // the left strip's last row
  const bool left_rows = strip > 0 && jl_left >= 1;
  const bool right_rows = lb >= 1 && c0 + F < (long long)la && c0 + F + 1 <= (long long)lb + d_hi;

  // entry e of a strip's hand-off column: two int4 at [2 e]
  const uint64_t hbase = wp.hand_off[pair];
  int4 *hand_out = reinterpret_cast<int4 *>(wp.handoff) + 2 * (hbase + (uint64_t)strip * (uint32_t)width);
  const int4 *hand_in = reinterpret_cast<const int4 *>(wp.handoff) + 2 * (hbase + (uint64_t)(strip ? strip - 1 : 0) * (uint32_t)width);

  if (!has_rows) {
    // no band cell in my columns.  A pair without any inner band cell gets its (empty) result from strip 0
    const long long colmin = max(1ll, 1ll + d_lo), colmax = min((long long)la, (long long)lb + d_hi);
    if (strip == 0 && (la == 0 || lb == 0 || colmin > colmax) && lane == 0) write_results(kp, pair, 0, ~0ull, 0ull);
    band_publish(word, front, kAllRows);
    return;
  }

  SpanSweep<CPL, SUBST, GENERAL> sw;
  const int g0 = lane * CPL;   // my first frame position
  // the frame of the row before my first: on column max(c0 + 1, d_lo) (d_lo > c0 + 1 only where jf = 1)
  const int fc_before = (int)max(c0 + 1, (long long)d_lo);
  sw.start_strip(p, k, sa_, la, (uint32_t)(fc_before - 1), (uint32_t)(fc_before - 1 + g0), lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  if (jf > 1) {   // the row above my first is outside the band in all my columns: stops of their own (the values are 0 already)
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      sw.Dx[c] = sw.Vx[c] = stop0((uint32_t)(fc_before + g0 + c), (uint32_t)(jf - 1));
      sw.Dy[c] = sw.Vy[c] = stop1((uint32_t)(fc_before + g0 + c), (uint32_t)(jf - 1));
    }
    sw.boundDx = stop0((uint32_t)(fc_before - 1), (uint32_t)(jf - 1));
    sw.boundDy = stop1((uint32_t)(fc_before - 1), (uint32_t)(jf - 1));
  }
  // of my columns left of the frame (wave-uniform): best value, its column and first row, that cell's span
  int ret_s = 0;
  uint32_t ret_col = 0, ret_row = 0, ret_x = 0, ret_y = 0;

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
          if (lane == 0) atomicCAS(wp.give_up, 0u, pair + 1u);
          band_publish(word, front, kAllRows);
          return;
        }
        left_done = (long long)need >= jl_left;
      }
      const uint32_t r = j + lane;
      code_b = 0;
      {   // no band cell left of the frame (strip 0: the border column): 0, not an A's, a stop of its own
        const uint32_t sx = (uint32_t)(max(c0 + 1, (long long)r + d_lo) - 1);
        in0 = make_int4(0, 0, 0, 0);
        in1 = make_int4((int)stop0(sx, r), (int)stop1(sx, r), (int)stop0(sx, r), (int)stop1(sx, r));
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
        sw.boundDx = (uint32_t)(zwins ? h1.x : h1.z);
        sw.boundDy = (uint32_t)(zwins ? h1.y : h1.w);
      }
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const long long jd = (long long)j + d_lo;
    const int fc = (int)max(c0 + 1, jd);
    if (jd >= c0 + 2) {   // the frame moves (wave-uniform): rule 1
      sw.boundX = read_lane(sw.X[0], 0);
      sw.boundDx = (uint32_t)read_lane((int)sw.Dx[0], 0);
      sw.boundDy = (uint32_t)read_lane((int)sw.Dy[0], 0);
      frame_shift(sw.X, 0);
      frame_shift(sw.Ap, 0);
      if constexpr (GENERAL) frame_shift(sw.Y, 0);
      frame_shift(sw.fa, 0);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, 0);
      frame_shift(sw.Dx, 0u); frame_shift(sw.Dy, 0u);
      frame_shift(sw.Vx, 0u); frame_shift(sw.Vy, 0u);
      // column fc - 1 leaves through lane 0
      const int s0 = read_lane(sw.bs[0], 0);
      if (s0 > ret_s) {
        ret_s = s0; ret_col = (uint32_t)(fc - 1);
        ret_row = (uint32_t)read_lane((int)sw.br[0], 0);
        ret_x = (uint32_t)read_lane((int)sw.bx[0], 0);
        ret_y = (uint32_t)read_lane((int)sw.by[0], 0);
      }
      frame_shift(sw.bs, 0);
      frame_shift(sw.br, 0u); frame_shift(sw.bx, 0u); frame_shift(sw.by, 0u);
    }
    // the cell above the band's right edge is outside the band: 0, and a stop of its own (rule 2)
    const long long jh = (long long)j + d_hi;
    const int ge = (int)min(jh - fc, (long long)F) - g0;
    const uint32_t edge_x = stop0((uint32_t)jh, j - 1), edge_y = stop1((uint32_t)jh, j - 1);
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? 0 : sw.X[c];
      sw.Ap[c] = edge ? 0 : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? 0 : sw.Y[c];
      sw.Vx[c] = edge ? edge_x : sw.Vx[c];
      sw.Vy[c] = edge ? edge_y : sw.Vy[c];
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
  unsigned long long key, span;
  // the last row's frame; a position that never held a band column of mine has kept 0
  sw.reduce_best((uint32_t)((int)max(c0 + 1, jl + d_lo) - 1 + g0), CPL, score, key, span);
  if (ret_s >= score && ret_s > 0) {   // a tie goes to the lower column: a retired one
    score = ret_s;
    key = ((unsigned long long)ret_col << 32) | ret_row;
    span = ((unsigned long long)ret_x << 32) | ret_y;
  }
  const uint64_t slot = wp.slot_off[pair] + strip;
  if (left_rows) {   // the best of the strips to my left: written before that strip's last publication
    if (!band_strip_wait(word - 1, front, kAllRows)) {
      if (lane == 0) atomicCAS(wp.give_up, 0u, pair + 1u);
      band_publish(word, front, kAllRows);
      return;
    }
    merge_left_best_span(wp.strip_best + kSpanBestWords * (slot - 1), score, key, span);
  }
  if (lane == 0) {
    if (!right_rows) {
      write_results(kp, pair, score, key, span);
    } else {
      const uint32_t ea = score > 0 ? (uint32_t)(key >> 32) : 0u, eb = score > 0 ? (uint32_t)key : 0u;
      uint4 *entry = reinterpret_cast<uint4 *>(wp.strip_best + kSpanBestWords * slot);
      entry[0] = make_uint4((uint32_t)score, ea, eb, 0u);
      entry[1] = make_uint4((uint32_t)(span >> 32), (uint32_t)span, 0u, 0u);
    }
  }
  band_publish(word, front, kAllRows);
}

template <int CPL>
static hipError_t launch_cpl(const SaBandSpanStripsParams &p, const dim3 grid, hipStream_t stream) {
  launch_by_scoring(p.s.b.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((band_span_strips_kernel<CPL, subst(), general()>), grid, dim3(kWave), table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace wide_span
}  // namespace sa

hipError_t sa_launch_band_span_strips(const SaBandSpanStripsParams &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  if (p.s.b.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.s.b.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (p.strips_per_pair == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  switch (strip_cols) {
    case 64: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_span::launch_cpl<1>(p, grid, stream);
    case 128: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_span::launch_cpl<2>(p, grid, stream);
    case 256: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_span::launch_cpl<4>(p, grid, stream);
    case 512: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_span::launch_cpl<8>(p, grid, stream);
  }
  return hipErrorInvalidValue;
}
