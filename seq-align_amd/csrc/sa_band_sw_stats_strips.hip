// sa_band_sw_stats_strips.hip -- wide banded SW statistics (seqalign_sw_stats_banded_wide): seqalign_sw_stats_banded's seven
// integers at any band width, one pair on many waves.  Two things that exist, crossed: the strip pipeline, the moving frame and
// the best cell merged from strip to strip of band_strips_kernel<CPL, SUBST, GENERAL, FILL = false, SW = true>
// (sa_band_strips.hip's header: the strips, their rows, the frame, the hand-off column, the tickets, the bounded wait and the
// give-up word) and the payload rules of the narrow statistics kernel (sa_band_stats.hip's header: the four rules) around
// SwStatSweep::row<BAND>.  DESIGN.md 3.27.
//
// band_sw_stats_strips_kernel<CPL, SUBST, GENERAL>: one workgroup = one wave = one (pair, strip), drawn by ticket.  Strip s owns
// columns c0 + 1 .. c0 + S, c0 = s S, S = 64 x CPL; its rows jf .. jl, fc(j) = max(c0 + 1, j + d_lo), fc_before = max(c0 + 1,
// d_lo), when the frame moves, ncol, left_rows / right_rows, the early exit of a strip without rows (strip 0 writes the seven
// zeros of a pair without inner band cells) and the progress, front and give-up words are band_strips_kernel's, to the letter.
// The payload rules, as they read per strip:
//   Shift (rule 1).  Ds / Dc / Vs / Vc and bs / br / bw0 / bw1 shift with X, Ap, Y, fa, arow; boundX / boundDs / boundDc become
//     lane 0's [0] from before the shift.  Lane 0's column retires into a wave-uniform best that keeps its two words (strict >: a
//     tie stays with the retired, lower column).  What enters on the right is a column past the strip's end, never a cell of
//     this strip: 0 in every word.
//   Outside the band is a stop that has counted nothing (rule 2): 0 in all three states, word 0 sw_stat_cell(x, y) of the cell
//     itself, word 1 = 0.  That is row jf - 1 in all its columns (row 0 for jf = 1, which start_strip has written so); position
//     g_e = j + d_hi - fc(j), the cell above the band's right edge, where it lies in the frame, in X, Ap, Y, Vs, Vc before every
//     row; the feed left of the frame wherever (c0, j) is no band cell -- on every row once the frame has moved, and strip 0's
//     border column on all its rows -- which is {0, 0, not from A, stop (fc(j) - 1, j), 0} in both payloads.
//   Left feed and up-left of a first row.  Strip s > 0, while (c0, j) is a band cell: the left strip's hand-off entry of the
//     row.  The up-left of a first row jf > 1 is (c0, jf - 1), on the band's right edge: hand-off entry 0, merged by row()'s
//     own boundary rule (A >= B > M via from_a).  Strip 0: the border cell (0, jf - 1), a stop of its own.
//   Hand-off.  Per row of the strip's last column c0 + S while that cell is in the band (rows c0 + S - d_hi .. c0 + S - d_lo):
//     StripSpanHandoff's content with x = word 0 and y = word 1, 32 bytes at entry [row - (c0 + S - d_hi)] of the strip's
//     `width` entries, moved 64 rows at a time and then published.  The column sits at frame position c0 + S - fc(j), which
//     moves: SwStatSweep::row<BAND, PICK> leaves that column's values in `out`, and they are read from the lane that holds it.
//   Best cell.  At the end of a strip reduce_best over the live columns, then the retired best first on a tie; then the wait for
//     the left strip's ~0 and merge_left_best_span (left wins a tie).  A strip with a right neighbour stores {score, end_a,
//     end_b, 0} {word 0, word 1, 0, 0} in its 32-byte best entry before its last publication, where the score kernel stores
//     its 16 bytes; the last strip of the run unpacks into the seven results as BandSwStatsFrame::write does.
//
// The 16-bit argument, per strip.  Word 0 is x | y << 16, right only while x <= 65 535; the host admits len_a, len_b <= 65 535,
// so a band cell (x, j) has 1 <= x <= len_a and its own word is exact.  A frame position right of len_a or right of the strip's
// end c0 + S can compute gx = fc(j) + g up to len_a + S - 1 > 65 535, and its word 0 is then garbage.  A band cell (x, j) of
// strip s, c0 < x <= min(len_a, c0 + S), reads exactly
//   - its up-left (x - 1, j - 1), on its own diagonal: a band cell of this strip, held one position to the left (frame standing)
//     or in the same position of the shifted arrays; for x = c0 + 1 the boundary, which row() derived from the feed of row
//     j - 1 (a band cell of the left strip or a stop in column c0 <= len_a), or the up-left rule above (hand-off entry 0, the
//     border cell, or start_strip's / the first-row stop (fc_before - 1, jf - 1), fc_before - 1 <= len_a); on the lowest diagonal
//     after a shift, lane 0's [0] from before the shift: the band cell (fc(j) - 1, j - 1) of this strip;
//   - the cell above it (x, j - 1), on diagonal x - j + 1 <= d_hi + 1: a band cell of this strip, or position g_e, which has just
//     been overwritten with sw_stat_cell(j + d_hi, j - 1), and x = j + d_hi <= len_a there since (x, j) is a band cell; on the
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
// Y, Vs, Vc; its Ds / Dc are read only by the cell below-right of it, one diagonal further right and no band cell.  A position
// right of min(len_a, c0 + S) never holds a cell of this strip: it is masked out of the best cell and the error key by ncol,
// and the hand-off reads column c0 + S only where c0 + S < len_a (right_rows) and the cell is in the band.  So no mask is
// needed and none is applied; tests/test_gpu_sw_stats_banded_wide.py runs both sequences at 65 535 letters over 1 024 strips
// with the last frames overhanging len_a to catch a mistake in this.  Word 1 needs no argument: matches + mismatches <=
// min(len_a, len_b) <= 65 535 in any cell.
// Nothing waits on a strip to its right; every path out of the kernel publishes ~0.
#include "sa_sw_stats.hpp"

namespace sa {
namespace wide_sw_stats {

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

// BandSwStatsFrame::write (sa_band_stats.hip): the seven results from the best cell's key and its two words
__device__ __forceinline__ void write_results(const SaBandSwStatsParams &kp, uint32_t pair, int score, unsigned long long key,
                                              unsigned long long words) {
  const bool hit = score > 0;
  const uint32_t ea = hit ? (uint32_t)(key >> 32) : 0u, eb = hit ? (uint32_t)key : 0u;
  const uint32_t w0 = hit ? (uint32_t)(words >> 32) : 0u, w1 = hit ? (uint32_t)words : 0u;
  const uint32_t pa = w0 & 0xffffu, pb = w0 >> 16;
  kp.b.score[pair] = hit ? score : 0;
  kp.pos_a[pair] = pa; kp.pos_b[pair] = pb;
  kp.len_a[pair] = ea - pa; kp.len_b[pair] = eb - pb;
  kp.matches[pair] = w1 & 0xffffu; kp.mismatches[pair] = w1 >> 16;
}

template <int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
band_sw_stats_strips_kernel(const SaBandSwStatsStripsParams wp) {
  const SaBandSwStatsParams &kp = wp.s;
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

  SwStatSweep<CPL, SUBST, GENERAL> sw;
  const int g0 = lane * CPL;   // my first frame position
  // the frame of the row before my first: on column max(c0 + 1, d_lo) (d_lo > c0 + 1 only where jf = 1)
  const int fc_before = (int)max(c0 + 1, (long long)d_lo);
  sw.start_strip(p, k, sa_, la, (uint32_t)(fc_before - 1), (uint32_t)(fc_before - 1 + g0), lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
  if (jf > 1) {   // the row above my first is outside the band in all my columns: stops of their own (the values are 0 already)
#pragma unroll
    for (int c = 0; c < CPL; ++c) sw.Ds[c] = sw.Vs[c] = sw_stat_cell((uint32_t)(fc_before + g0 + c), (uint32_t)(jf - 1));
    sw.boundDs = sw_stat_cell((uint32_t)(fc_before - 1), (uint32_t)(jf - 1));
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
          if (lane == 0) atomicCAS(wp.give_up, 0u, pair + 1u);
          band_publish(word, front, kAllRows);
          return;
        }
        left_done = (long long)need >= jl_left;
      }
      const uint32_t r = j + lane;
      code_b = 0;
      {   // no band cell left of the frame (strip 0: the border column): 0, not an A's, a stop of its own that has counted nothing
        const uint32_t stop = sw_stat_cell((uint32_t)(max(c0 + 1, (long long)r + d_lo) - 1), r);
        in0 = make_int4(0, 0, 0, 0);
        in1 = make_int4((int)stop, 0, (int)stop, 0);
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
        sw.boundDs = (uint32_t)(zwins ? h1.x : h1.z);
        sw.boundDc = (uint32_t)(zwins ? h1.y : h1.w);
      }
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const long long jd = (long long)j + d_lo;
    const int fc = (int)max(c0 + 1, jd);
    if (jd >= c0 + 2) {   // the frame moves (wave-uniform): rule 1
      sw.boundX = read_lane(sw.X[0], 0);
      sw.boundDs = (uint32_t)read_lane((int)sw.Ds[0], 0);
      sw.boundDc = (uint32_t)read_lane((int)sw.Dc[0], 0);
      frame_shift(sw.X, 0);
      frame_shift(sw.Ap, 0);
      if constexpr (GENERAL) frame_shift(sw.Y, 0);
      frame_shift(sw.fa, 0);
      if constexpr (SUBST != SA_SUBST_SIMPLE) frame_shift(sw.arow, 0);
      frame_shift(sw.Ds, 0u); frame_shift(sw.Dc, 0u);
      frame_shift(sw.Vs, 0u); frame_shift(sw.Vc, 0u);
      // column fc - 1 leaves through lane 0
      const int s0 = read_lane(sw.bs[0], 0);
      if (s0 > ret_s) {
        ret_s = s0; ret_col = (uint32_t)(fc - 1);
        ret_row = (uint32_t)read_lane((int)sw.br[0], 0);
        ret_0 = (uint32_t)read_lane((int)sw.bw0[0], 0);
        ret_1 = (uint32_t)read_lane((int)sw.bw1[0], 0);
      }
      frame_shift(sw.bs, 0);
      frame_shift(sw.br, 0u); frame_shift(sw.bw0, 0u); frame_shift(sw.bw1, 0u);
    }
    // the cell above the band's right edge is outside the band: 0, and a stop of its own (rule 2)
    const long long jh = (long long)j + d_hi;
    const int ge = (int)min(jh - fc, (long long)F) - g0;
    const uint32_t edge_stop = sw_stat_cell((uint32_t)jh, j - 1);
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool edge = (c == ge);
      sw.X[c] = edge ? 0 : sw.X[c];
      sw.Ap[c] = edge ? 0 : sw.Ap[c];
      if constexpr (GENERAL) sw.Y[c] = edge ? 0 : sw.Y[c];
      sw.Vs[c] = edge ? edge_stop : sw.Vs[c];
      sw.Vc[c] = edge ? 0u : sw.Vc[c];
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
  const uint64_t slot = wp.slot_off[pair] + strip;
  if (left_rows) {   // the best of the strips to my left: written before that strip's last publication
    if (!band_strip_wait(word - 1, front, kAllRows)) {
      if (lane == 0) atomicCAS(wp.give_up, 0u, pair + 1u);
      band_publish(word, front, kAllRows);
      return;
    }
    merge_left_best_span(wp.strip_best + kSpanBestWords * (slot - 1), score, key, words);
  }
  if (lane == 0) {
    if (!right_rows) {
      write_results(kp, pair, score, key, words);
    } else {
      const uint32_t ea = score > 0 ? (uint32_t)(key >> 32) : 0u, eb = score > 0 ? (uint32_t)key : 0u;
      uint4 *entry = reinterpret_cast<uint4 *>(wp.strip_best + kSpanBestWords * slot);
      entry[0] = make_uint4((uint32_t)score, ea, eb, 0u);
      entry[1] = make_uint4((uint32_t)(words >> 32), (uint32_t)words, 0u, 0u);
    }
  }
  band_publish(word, front, kAllRows);
}

template <int CPL>
static hipError_t launch_cpl(const SaBandSwStatsStripsParams &p, const dim3 grid, hipStream_t stream) {
  launch_by_scoring(p.s.b.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((band_sw_stats_strips_kernel<CPL, subst(), general()>), grid, dim3(kWave), table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace wide_sw_stats
}  // namespace sa

hipError_t sa_launch_band_sw_stats_strips(const SaBandSwStatsStripsParams &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  if (p.s.b.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.s.b.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (p.strips_per_pair == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  switch (strip_cols) {
    case 64: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_sw_stats::launch_cpl<1>(p, grid, stream);
    case 128: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_sw_stats::launch_cpl<2>(p, grid, stream);
    case 256: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_sw_stats::launch_cpl<4>(p, grid, stream);
    case 512: sa_record_launch_ext(SEQALIGN_KX_BAND_SCORE, items); return sa::wide_sw_stats::launch_cpl<8>(p, grid, stream);
  }
  return hipErrorInvalidValue;
}
