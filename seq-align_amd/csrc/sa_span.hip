// sa_span.hip -- SW hit spans: the best local hit's score, start and end of each pair, no matrices, no traceback, any length
// (seqalign_sw_span_batch).  sa_score.hip's SW sweep with one thing more carried beside the three values of a cell: for each
// of its states S in {match, gap_a, gap_b} the SPAN of (cell, S) -- the cell in which the reference's walk
// (alignment_reverse_move, tie order GAP_A, GAP_B, MATCH; sa_trace_common.hpp) stops when it starts there.  DESIGN.md 3.18:
//   span(cell, S) = the cell itself where value(cell, S) <= 0 or the cell is on the border,
//                   else span(predecessor the walker picks).
// The walker's no_gaps_in_a / _b predicates never change a span: a state they exclude holds the floor 0, and where a 0 still
// ties for the maximum every state of that predecessor holds 0, so each of them stops in that very cell.
//
// What crosses a row, per column: two merged spans of the previous row's cell, both chosen when that row ends --
//   D  the diagonal feed of M(x+1, y+1): the span of the argmax of A, B, M, priority A > B > M;
//   V  the vertical feed of A(x, y+1):   A + ext first, then B, then M, each + open1.
// Within a row gap_b's span rides the (max,+) scan: the scan's element is {value, span, one bit}, its operator the maximum
// by (value, tie key).  A candidate for B(g) enters the chain at a column k <= g; the walker, going left from g, takes an
// opening from A as soon as it meets one, walks on while the chain continues, stops in a gap_b cell that holds 0 (possible
// only with gap_extend > 0: the floor is a source), and takes an opening from M only when nothing lies further left.  As a
// total order on candidates of equal value (tests/test_sw_span_argument_cpu.py checks it against the step-by-step walk):
//   opening from M at k: -k - 2   (the earliest wins, below everything else)
//   the chain coming in from the strip to the left: -1
//   opening from A at k: 2k       (the latest wins)
//   the floor at k: 2k + 1        (beats what lies at or left of it, loses to a later opening from A)
// The kernel never forms the key.  It only ever merges a candidate (or a run of them) L with one that lies to its RIGHT, R,
// and between such two the order says: R wins a tie unless R is an opening from M.  So a candidate carries one bit, nm = "not
// an opening from M", and the merge is  L.v >= R.v + R.nm ? L : R  -- one add and one compare.
//
// span_rows_kernel: rows of up to 512 columns, one wave per pair (1 .. 6 or 8 columns per lane), 4 pairs per workgroup.
// span_strips_kernel: wider rows, the strips pipeline of sa_strips.hpp -- the hand-off per row and strip is 32 bytes
// (StripSpanHandoff: max(M, A) and B of the strip's last column, their spans, and whether max(M, A) came from A), the best
// cell so far travels with its span (merge_left_best_span).  Both are recorded as "score_rows" / "score_strips".
#include "sa_strips.hpp"

namespace sa {

constexpr int kSpanStripCPL = 8;   // 512 columns per strip, as sa_score.hip
constexpr uint32_t kSpanStripCols = kWave * kSpanStripCPL;

// one candidate of the gap_b chain: value (de-trended, sa_rowsweep.hpp), nm (header comment), the span it brings
struct SpanCand {
  int v, nm;
  uint32_t x, y;
};
// l lies left of r
__device__ __forceinline__ SpanCand span_merge(const SpanCand &l, const SpanCand &r) {
  const bool left = l.v >= addw(r.v, r.nm);
  return SpanCand{left ? l.v : r.v, left ? l.nm : r.nm, left ? l.x : r.x, left ? l.y : r.y};
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ SpanCand span_dpp(const SpanCand &u) {   // lanes without a source: max's identity
  return SpanCand{dpp_mov<CTRL, ROW_MASK>(INT32_MIN, u.v), dpp_mov<CTRL, ROW_MASK>(0, u.nm),
                  (uint32_t)dpp_mov<CTRL, ROW_MASK>(0, (int)u.x), (uint32_t)dpp_mov<CTRL, ROW_MASK>(0, (int)u.y)};
}
// wave_scan_max (sa_rowsweep.hpp) over candidates: what arrives comes from lower lanes, so from the left
__device__ __forceinline__ SpanCand wave_scan_span(SpanCand u) {
  u = span_merge(span_dpp<0x111, 0xf>(u), u);   // row_shr:1
  u = span_merge(span_dpp<0x112, 0xf>(u), u);   // row_shr:2
  u = span_merge(span_dpp<0x114, 0xf>(u), u);   // row_shr:4
  u = span_merge(span_dpp<0x118, 0xf>(u), u);   // row_shr:8
  u = span_merge(span_dpp<0x142, 0xa>(u), u);   // row_bcast:15 -> rows 1,3
  u = span_merge(span_dpp<0x143, 0xc>(u), u);   // row_bcast:31 -> rows 2,3
  return u;
}

// what a strip reads of the cell left of it on one row (strip 0: the border column, all 0 and its own span)
struct SpanFeed {
  int z, b, from_a;            // max(M, A), B; whether max(M, A) is A's (A >= M)
  uint32_t zx, zy, bx, by;     // the spans of that state and of B
};

// RowSweep's SW arithmetic (floor 0, border 0) with the spans beside it.  Column c of a lane is matrix column col0 + c + 1.
template <int CPL, int SUBST, bool GENERAL>
struct SpanSweep {
  int fa[CPL], arow[CPL];
  int X[CPL], Ap[CPL];
  int Y[GENERAL ? CPL : 1];
  int c1[CPL], c2[CPL], c3[CPL];
  uint32_t Dx[CPL], Dy[CPL], Vx[CPL], Vy[CPL];   // previous row: the diagonal and the vertical feed (header comment)
  int boundX;                                    // max3 of the cell left of the strip on the previous row ...
  uint32_t boundDx, boundDy;                     // ... and its diagonal feed
  int trend0;
  unsigned long long err = ~0ull;
  // the running best of match_scores per column (BestCells), with the span of that cell's match state
  int bs[CPL];
  uint32_t br[CPL], bx[CPL], by[CPL];

  __device__ __forceinline__ void start_strip(const SaFillParams &p, const SweepConsts &k, const uint8_t *__restrict__ seq_a,
                                              uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    trend0 = k.ext > 0 ? (kWave * CPL) * k.ext : 0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const uint32_t idx = col0 + c;
      const int code = idx < la ? (int)p.code[seq_a[idx]] : 0;
      fa[c] = code & 0xff;
      arow[c] = (code >> 8) * k.K;
      X[c] = 0; Ap[c] = 0;
      if constexpr (GENERAL) Y[c] = 0;
      Dx[c] = Vx[c] = idx + 1; Dy[c] = Vy[c] = 0;   // row 0 holds 0: every walk that reaches it stops there
      const int g_ext = (lane * CPL + c) * k.ext - trend0;
      c1[c] = k.open1 - g_ext;
      c2[c] = -g_ext;
      c3[c] = g_ext;
      bs[c] = 0; br[c] = 0; bx[c] = 0; by[c] = 0;
    }
    boundX = 0; boundDx = i0; boundDy = 0;
  }

  // Row j.  f: the cell left of the strip on this row.  Leaves the last column's hand-off in `out` (lane 63's is the strip's).
  __device__ __forceinline__ void row(const SweepConsts &k, uint32_t j, uint32_t lb, uint32_t la, uint32_t W, int lane,
                                      uint32_t col0, int ncol, int code_b, const SpanFeed &f, SpanFeed &out) {
    int xd = wave_shr1(X[CPL - 1], boundX);
    uint32_t dx = (uint32_t)wave_shr1((int)Dx[CPL - 1], (int)boundDx), dy = (uint32_t)wave_shr1((int)Dy[CPL - 1], (int)boundDy);
    {   // the boundary cell of this row, for the next one: A > B > M over {max(M, A) and whose it is, B}
      boundX = max(f.z, f.b);
      const bool zwins = f.from_a ? f.z >= f.b : f.z > f.b;
      boundDx = zwins ? f.zx : f.bx;
      boundDy = zwins ? f.zy : f.by;
    }
    int mv[CPL], av[CPL], bv[CPL];
    uint32_t mx[CPL], my[CPL], ax[CPL], ay[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const uint32_t gx = col0 + c + 1;
      const int s = subst_score<SUBST>(fa[c], arow[c], code_b, k.table, k.gen_eq, k.gen_ne);
      int m, a;
      bool a_free = false;   // gap_a of the last column under no_end_gap_penalty: max3 of the cell above, no penalty
      if constexpr (GENERAL) {
        const int a_norm = max3i(addw(Y[c], k.open1), addw(Ap[c], k.ext), 0);
        m = (s == SA_S_BLOCKED) ? 0 : max(addw(xd, s), 0);
        if (s == SA_S_UNKNOWN && c < ncol) {
          m = 0;
          err = min(err, (unsigned long long)j * W + gx);
        }
        const bool last_col = (gx == la);
        a_free = last_col && k.no_end;
        a = a_free ? max(Y[c], Ap[c]) : (!k.no_gaps_a || last_col) ? a_norm : 0;
      } else {
        m = max(addw(xd, s), 0);
        a = max3i(addw(X[c], k.open1), addw(Ap[c], k.ext), 0);
      }
      mx[c] = m > 0 ? dx : gx; my[c] = m > 0 ? dy : j;
      ax[c] = a > 0 ? (a_free ? Dx[c] : Vx[c]) : gx;
      ay[c] = a > 0 ? (a_free ? Dy[c] : Vy[c]) : j;
      xd = X[c]; dx = Dx[c]; dy = Dy[c];
      mv[c] = m; av[c] = a;
      const bool up = m > bs[c];   // strict: the first (lowest) row keeps a tie
      bs[c] = up ? m : bs[c]; br[c] = up ? j : br[c]; bx[c] = up ? mx[c] : bx[c]; by[c] = up ? my[c] : by[c];
    }

    // gap_b
    bool free_row = false, forced = false;
    if constexpr (GENERAL) {
      const bool last_row = (j == lb);
      free_row = last_row && k.no_end;
      forced = k.no_gaps_b && !last_row;
    }
    uint32_t bxs[CPL], bys[CPL];
    if (forced) {
#pragma unroll
      for (int c = 0; c < CPL; ++c) { bv[c] = 0; bxs[c] = col0 + c + 1; bys[c] = j; }
    } else {
      // max(M, A) of the column to my left, whose it is, and its span
      const bool la_from_a = av[CPL - 1] >= mv[CPL - 1];
      int zl = wave_shr1(max(mv[CPL - 1], av[CPL - 1]), f.z);
      int zl_a = wave_shr1((int)la_from_a, f.from_a);
      uint32_t zlx = (uint32_t)wave_shr1((int)(la_from_a ? ax[CPL - 1] : mx[CPL - 1]), (int)f.zx);
      uint32_t zly = (uint32_t)wave_shr1((int)(la_from_a ? ay[CPL - 1] : my[CPL - 1]), (int)f.zy);
      SpanCand P[CPL];
      const bool floor_pays = !free_row && k.ext > 0;   // only then can the floor of a cell feed a positive cell to its right
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        SpanCand w{free_row ? zl : addw(zl, c1[c]), zl_a, zlx, zly};
        if (floor_pays) {   // the floor of this very cell: it wins a tie with the opening that enters here
          const bool fl = c2[c] >= w.v;
          w = SpanCand{fl ? c2[c] : w.v, fl ? 1 : w.nm, fl ? col0 + c + 1 : w.x, fl ? j : w.y};
        }
        if (c == 0) {   // lane 0 continues the previous strip's chain: B(left) + ext, de-trended at g = 0
          const SpanCand carry{free_row ? f.b : addw(addw(f.b, k.ext), trend0), 1, f.bx, f.by};
          const SpanCand wc = span_merge(carry, w);
          const bool l0 = lane == 0;   // (member by member: a select between two structs goes through memory)
          w = SpanCand{l0 ? wc.v : w.v, l0 ? wc.nm : w.nm, l0 ? wc.x : w.x, l0 ? wc.y : w.y};
        }
        P[c] = (c == 0) ? w : span_merge(P[c - 1], w);
        const bool fa_ = av[c] >= mv[c];
        zl = max(mv[c], av[c]); zl_a = fa_;
        zlx = fa_ ? ax[c] : mx[c]; zly = fa_ ? ay[c] : my[c];
      }
      const SpanCand incl = wave_scan_span(P[CPL - 1]);
      const SpanCand e{wave_shr1(incl.v, INT32_MIN), 0, (uint32_t)wave_shr1((int)incl.x, 0), (uint32_t)wave_shr1((int)incl.y, 0)};
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const SpanCand pm = span_merge(e, P[c]);
        bv[c] = max(free_row ? pm.v : addw(pm.v, c3[c]), 0);   // (the clamp: the floor is not among the candidates unless it pays)
        bxs[c] = bv[c] > 0 ? pm.x : col0 + c + 1;
        bys[c] = bv[c] > 0 ? pm.y : j;
      }
    }

    // the feeds of the next row
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int mb = max(mv[c], bv[c]);
      const bool b_over_m = bv[c] >= mv[c];
      const uint32_t lx = b_over_m ? bxs[c] : mx[c], ly = b_over_m ? bys[c] : my[c];
      const bool d_a = av[c] >= mb, v_a = addw(av[c], k.ext) >= addw(mb, k.open1);
      Dx[c] = d_a ? ax[c] : lx; Dy[c] = d_a ? ay[c] : ly;
      Vx[c] = v_a ? ax[c] : lx; Vy[c] = v_a ? ay[c] : ly;
      X[c] = max(av[c], mb);
      if constexpr (GENERAL) Y[c] = mb;
      Ap[c] = av[c];
    }
    const bool o_a = av[CPL - 1] >= mv[CPL - 1];
    out.z = max(mv[CPL - 1], av[CPL - 1]); out.b = bv[CPL - 1]; out.from_a = o_a;
    out.zx = o_a ? ax[CPL - 1] : mx[CPL - 1]; out.zy = o_a ? ay[CPL - 1] : my[CPL - 1];
    out.bx = bxs[CPL - 1]; out.by = bys[CPL - 1];
  }

  __device__ __forceinline__ unsigned long long reduce_err() {
    unsigned long long e = err;
    if constexpr (GENERAL) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) e = min(e, __shfl_xor(e, o));
    }
    return e;
  }

  // BestCells::reduce, and the span of the winning cell: {score, (column << 32) | row, (pos_a << 32) | pos_b}
  __device__ __forceinline__ void reduce_best(uint32_t col0, int ncol, int &score, unsigned long long &key,
                                              unsigned long long &span) const {
    int b = 0;
    unsigned long long kb = ~0ull, sb = 0;
#pragma unroll
    for (int c = 0; c < CPL; ++c)   // c ascending, strict >: the lowest column wins a tie
      if (c < ncol && bs[c] > b) {
        b = bs[c];
        kb = ((unsigned long long)(col0 + c + 1) << 32) | br[c];
        sb = ((unsigned long long)bx[c] << 32) | by[c];
      }
    score = wave_max_i32(b);
    const unsigned long long mine = (b == score && score > 0) ? kb : ~0ull;
    key = wave_min_u64(mine);
    span = wave_min_u64((mine == key && score > 0) ? sb : ~0ull);   // one lane holds the key
  }
};

__device__ __forceinline__ void span_write(const SaSpanParams &sp, uint64_t at, int score, unsigned long long key,
                                           unsigned long long span) {
  const bool hit = score > 0;
  const uint32_t ea = hit ? (uint32_t)(key >> 32) : 0u, eb = hit ? (uint32_t)key : 0u;
  const uint32_t pa = hit ? (uint32_t)(span >> 32) : 0u, pb = hit ? (uint32_t)span : 0u;
  sp.score[at] = hit ? score : 0;
  sp.pos_a[at] = pa; sp.pos_b[at] = pb;
  sp.len_a[at] = ea - pa; sp.len_b[at] = eb - pb;
}

template <int CPL, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
span_rows_kernel(const SaSpanParams sp) {
  const SaFillParams &p = sp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t pair = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (pair >= p.n_pairs) return;   // wave-uniform, after the only barrier

  const uint32_t la = p.len_a[pair], lb = p.len_b[pair];
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[pair];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[pair];
  const uint32_t W = la + 1;
  const SweepConsts k(p, table);

  SpanSweep<CPL, SUBST, GENERAL> sw;
  const uint32_t col0 = lane * CPL;
  const int ncol = max(0, min(CPL, (int)la - lane * CPL));
  sw.start_strip(p, k, sa_, la, 0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)

  int code = 0;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {   // every 64 rows: lane t fetches seq_b's code for row j + t
      const uint32_t r = j + lane;
      if (r <= lb) code = p.code[sb_[r - 1]];
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const SpanFeed f{0, 0, 0, 0u, j, 0u, j};   // the border column: cell (0, j) holds 0
    SpanFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  int score;
  unsigned long long key, span;
  sw.reduce_best(col0, ncol, score, key, span);
  if (lane == 0) {
    span_write(sp, pair, score, key, span);
    p.status[pair] = err;
    if (err != ~0ull) atomicOr(sp.err_flag, 1u);
  }
}

template <int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
span_strips_kernel(const SaSpanParams sp) {
  constexpr int CPL = kSpanStripCPL;
  const SaFillParams &p = sp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x;
  const uint32_t spp = sp.strips_per_pair;
  uint32_t strip, pair;
  strip_of_ticket(strip_ticket(sp.progress + (uint64_t)gridDim.x), spp, strip, pair);
  if (pair >= p.n_pairs) return;

  const uint32_t la = p.len_a[pair], lb = p.len_b[pair];
  const uint32_t i0 = strip * kSpanStripCols;
  if (i0 >= la && strip != 0) return;   // this pair has fewer strips
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[pair];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[pair];
  const uint32_t W = la + 1;
  const uint64_t slot = (uint64_t)pair * spp + strip;   // my progress word / strip_best entry
  uint32_t *done = sp.progress + (uint64_t)pair * spp;  // done[s] = rows strip s has handed over
  const uint64_t rows = (uint64_t)lb + 1;
  int32_t *hand_out = sp.handoff + kSpanHandoffInts * (sp.handoff_off[pair] + (uint64_t)strip * rows);
  const int32_t *hand_in = sp.handoff + kSpanHandoffInts * (sp.handoff_off[pair] + (uint64_t)(strip ? strip - 1 : 0) * rows);

  const SweepConsts k(p, table);
  const uint32_t cols = (i0 < la) ? min(kSpanStripCols, la - i0) : 0;
  const bool last_strip = i0 + kSpanStripCols >= la;
  const uint32_t col0 = i0 + lane * CPL;
  const int ncol = max(0, min(CPL, (int)cols - lane * CPL));
  SpanSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, sa_, la, i0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);

  StripSpanHandoff h;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {
      // rows j .. j + 63 of the strip to my left must have been handed over
      if (strip > 0) strip_wait(done + strip - 1, min(j + kWave - 1, lb));
      h.load(p, sb_, lb, strip, i0, hand_in, j + lane);
    }
    const SpanFeed f{read_lane(h.in0.x, q), read_lane(h.in0.y, q), read_lane(h.in0.z, q),
                     (uint32_t)read_lane(h.in1.x, q), (uint32_t)read_lane(h.in1.y, q),
                     (uint32_t)read_lane(h.in1.z, q), (uint32_t)read_lane(h.in1.w, q)};
    SpanFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(h.code, q), f, out);
    if (!last_strip) {   // a strip that is not the last is full: lane 63's last column is the strip's
      const int4 o0 = make_int4(read_lane(out.z, kWave - 1), read_lane(out.b, kWave - 1), read_lane(out.from_a, kWave - 1), 0);
      const int4 o1 = make_int4(read_lane((int)out.zx, kWave - 1), read_lane((int)out.zy, kWave - 1),
                                read_lane((int)out.bx, kWave - 1), read_lane((int)out.by, kWave - 1));
      h.keep(o0, o1, hand_out, done + strip, lane, q, j, lb);
    }
  }

  const unsigned long long err = sw.reduce_err();
  if (lane == 0 && err != ~0ull) {
    atomicMin(reinterpret_cast<unsigned long long *>(p.status + pair), err);
    atomicOr(sp.err_flag, 1u);
  }
  int score;
  unsigned long long key, span;
  sw.reduce_best(col0, ncol, score, key, span);
  if (strip > 0 && lb > 0) merge_left_best_span(sp.strip_best + kSpanBestWords * (slot - 1), score, key, span);
  if (lane == 0) {
    if (last_strip) {
      span_write(sp, pair, score, key, span);
    } else {
      uint4 *entry = reinterpret_cast<uint4 *>(sp.strip_best + kSpanBestWords * slot);
      entry[0] = make_uint4((uint32_t)score, (uint32_t)(key >> 32), (uint32_t)key, 0u);
      entry[1] = make_uint4((uint32_t)(span >> 32), (uint32_t)span, 0u, 0u);
    }
  }
  if (!last_strip && lb > 0) strip_publish(done + strip, lb);   // the last rows (and the best cell so far)
}

template <int CPL>
static hipError_t launch_span_rows_cpl(const SaSpanParams &p, hipStream_t stream) {
  const dim3 grid((p.f.n_pairs + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((span_rows_kernel<CPL, subst(), general()>), grid, block, table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

uint32_t sa_span_strips_per_pair(uint32_t max_len_a) {
  return max_len_a ? (uint32_t)(((uint64_t)max_len_a + sa::kSpanStripCols - 1) / sa::kSpanStripCols) : 1;
}

hipError_t sa_launch_span_rows(const SaSpanParams &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_ROWS, p.f.n_pairs);
  return sa::launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(sa::columns_per_lane(max_len_a), [&](auto cpl) { return sa::launch_span_rows_cpl<cpl()>(p, stream); });
}

hipError_t sa_launch_span_strips(const SaSpanParams &p, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_STRIPS, p.f.n_pairs);
  sa::launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((sa::span_strips_kernel<subst(), general()>), dim3((unsigned)blocks), dim3(sa::kWave),
                       table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}
