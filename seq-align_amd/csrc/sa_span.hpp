// sa_span.hpp -- the arithmetic of the SW hit-span sweeps: SpanCand and its merge, the (max,+) scan over candidates, SpanFeed,
// SpanSweep (one matrix row per step, the spans beside the scores) and span_write.  The definition and the tie argument are in
// sa_span.hip's header; the kernels that use this are sa_span.hip's (whole matrices) and sa_band_span.hip's (a band).
#pragma once
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
    trend0 = k.ext > 0 ? mulw(kWave * CPL, k.ext) : 0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const uint32_t idx = col0 + c;
      const int code = idx < la ? (int)p.code[seq_a[idx]] : 0;
      fa[c] = code & 0xff;
      arow[c] = (code >> 8) * k.K;
      X[c] = 0; Ap[c] = 0;
      if constexpr (GENERAL) Y[c] = 0;
      Dx[c] = Vx[c] = idx + 1; Dy[c] = Vy[c] = 0;   // row 0 holds 0: every walk that reaches it stops there
      const int g_ext = subw(mulw(lane * CPL + c, k.ext), trend0);
      c1[c] = subw(k.open1, g_ext);
      c2[c] = subw(0, g_ext);
      c3[c] = g_ext;
      bs[c] = 0; br[c] = 0; bx[c] = 0; by[c] = 0;
    }
    boundX = 0; boundDx = i0; boundDy = 0;
  }

  // Row j.  f: the cell left of the strip on this row.  Leaves the last column's hand-off in `out` (lane 63's is the strip's).
  // BAND (sa_band_span.hip): ncol changes from row to row, so the running best takes a cell only while its column is in the band.
  // PICK (band_payload_strips_kernel, sa_band_frame.hpp, where the strip's last column moves through the frame): `out` is column `pick` of the
  // lane instead of its last.
  template <bool BAND = false, bool PICK = false>
  __device__ __forceinline__ void row(const SweepConsts &k, uint32_t j, uint32_t lb, uint32_t la, uint32_t W, int lane,
                                      uint32_t col0, int ncol, int code_b, const SpanFeed &f, SpanFeed &out, int pick = CPL - 1) {
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
      const bool up = (!BAND || c < ncol) && m > bs[c];   // strict: the first (lowest) row keeps a tie
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
    if constexpr (!PICK) {
      const bool o_a = av[CPL - 1] >= mv[CPL - 1];
      out.z = max(mv[CPL - 1], av[CPL - 1]); out.b = bv[CPL - 1]; out.from_a = o_a;
      out.zx = o_a ? ax[CPL - 1] : mx[CPL - 1]; out.zy = o_a ? ay[CPL - 1] : my[CPL - 1];
      out.bx = bxs[CPL - 1]; out.by = bys[CPL - 1];
    } else {
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (c == pick || CPL == 1) {
          const bool o_a = av[c] >= mv[c];
          out.z = max(mv[c], av[c]); out.b = bv[c]; out.from_a = o_a;
          out.zx = o_a ? ax[c] : mx[c]; out.zy = o_a ? ay[c] : my[c];
          out.bx = bxs[c]; out.by = bys[c];
        }
    }
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

}  // namespace sa
