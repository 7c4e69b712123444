// sa_sw_gaps.hpp -- the arithmetic of the SW gap-run sweeps (sa_sw_gaps.hip, sa_band_gaps.hip): SwGapSweep, one matrix row per
// step, SwCountSweep's SW values and tie rules (sa_sw_counts.hpp) with another meaning in the two payload words beside each of
// match, gap_a and gap_b:
//   word 0  x = gap_runs_a    the maximal runs of gap_a columns ('-' in string a) of the walk that starts in that state,
//   word 1  y = gap_runs_b    its maximal runs of gap_b columns ('-' in string b).
// Both are full 32-bit words and there is no stop cell: a walk has fewer than len_a + len_b < 2^31 columns, so neither word can
// wrap at any length, and a state that stops holds (0, 0) wherever it stops.  A run is counted at its FIRST column in forward
// order, which is the last gap state the walk passes before it leaves the run: a gap state adds one unless the predecessor the
// walker picks is the same gap state and is not itself a stop.  Every feed, hand-off and stop stays in RAW form (the pair of the
// state it names, a stop (0, 0)); the increment is decided in the consuming cell:
//   gap_a   + 1 in x unless the extension wins the vertical feed and the gap_a above is > 0;
//   gap_b   every opening candidate of the row scan carries its source's pair + 1 in y, the floor candidate (a stop) carries
//           (0, 1) for the cells that extend out of it, the carry from the left strip or border + 1 iff its B is <= 0; a cell
//           whose own value is <= 0 holds (0, 0).
// Score and end cell come from the best cell's key, as in every SW sweep.  The scan's element, its merge and the feed of a strip
// are sa_span.hpp's: in a SpanCand / SpanFeed here x is word 0 and y word 1, two opaque words.
// The definition and the tie argument are in sa_sw_gaps.hip's header.
#pragma once
#include "sa_span.hpp"

namespace sa {

template <int CPL, int SUBST, bool GENERAL>
struct SwGapSweep {
  int fa[CPL], arow[CPL];
  int X[CPL], Ap[CPL];
  int Y[GENERAL ? CPL : 1];
  int c1[CPL], c2[CPL], c3[CPL];
  uint32_t Da[CPL], Db[CPL], Va[CPL], Vb[CPL];   // previous row: the diagonal and the vertical feed, {gap_runs_a, gap_runs_b} each
  int boundX;                                    // max3 of the cell left of the strip on the previous row ...
  uint32_t boundDa, boundDb;                     // ... and its diagonal feed
  int trend0;
  unsigned long long err = ~0ull;
  // the running best of match_scores per column (BestCells), with the two run counts of that cell's match state
  int bs[CPL];
  uint32_t br[CPL], bw0[CPL], bw1[CPL];

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
      Da[c] = Va[c] = 0; Db[c] = Vb[c] = 0;   // row 0 holds 0: every walk that reaches it stops there, no run counted
      const int g_ext = subw(mulw(lane * CPL + c, k.ext), trend0);
      c1[c] = subw(k.open1, g_ext);
      c2[c] = subw(0, g_ext);
      c3[c] = g_ext;
      bs[c] = 0; br[c] = 0; bw0[c] = 0; bw1[c] = 0;
    }
    (void)i0;
    boundX = 0; boundDa = 0; boundDb = 0;
  }

  // Row j.  f: the cell left of the strip on this row.  Leaves the last column's hand-off in `out` (lane 63's is the strip's).
  // BAND (sa_band_gaps.hip): ncol changes from row to row, so the running best takes a cell only while its column is in the band.
  // PICK (band_payload_strips_kernel, sa_band_frame.hpp, where the strip's last column moves through the frame): `out` is column `pick` of the
  // lane instead of its last.
  template <bool BAND = false, bool PICK = false>
  __device__ __forceinline__ void row(const SweepConsts &k, uint32_t j, uint32_t lb, uint32_t la, uint32_t W, int lane,
                                      uint32_t col0, int ncol, int code_b, const SpanFeed &f, SpanFeed &out, int pick = CPL - 1) {
    int xd = wave_shr1(X[CPL - 1], boundX);
    uint32_t dm = (uint32_t)wave_shr1((int)Da[CPL - 1], (int)boundDa), dn = (uint32_t)wave_shr1((int)Db[CPL - 1], (int)boundDb);
    {   // the boundary cell of this row, for the next one: A > B > M over {max(M, A) and whose it is, B}
      boundX = max(f.z, f.b);
      const bool zwins = f.from_a ? f.z >= f.b : f.z > f.b;
      boundDa = zwins ? f.zx : f.bx;
      boundDb = zwins ? f.zy : f.by;
    }
    int mv[CPL], av[CPL], bv[CPL];
    uint32_t mm[CPL], mn[CPL], am[CPL], an[CPL];
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
      // the match state adds nothing; gap_a opens a run here unless it extends a gap_a above that is not a stop
      bool a_ext;
      if constexpr (GENERAL) a_ext = a_free ? Ap[c] >= Y[c] : addw(Ap[c], k.ext) >= addw(Y[c], k.open1);
      else a_ext = addw(Ap[c], k.ext) >= addw(X[c], k.open1);   // (gap_open <= 0 here: X stands for max(M, B) as in the V feed)
      const uint32_t a_inc = (a_ext && Ap[c] > 0) ? 0u : 1u;
      mm[c] = m > 0 ? dm : 0u;
      mn[c] = m > 0 ? dn : 0u;
      am[c] = a > 0 ? (a_free ? Da[c] : Va[c]) + a_inc : 0u;
      an[c] = a > 0 ? (a_free ? Db[c] : Vb[c]) : 0u;
      xd = X[c]; dm = Da[c]; dn = Db[c];
      mv[c] = m; av[c] = a;
      const bool up = (!BAND || c < ncol) && m > bs[c];   // strict: the first (lowest) row keeps a tie
      bs[c] = up ? m : bs[c]; br[c] = up ? j : br[c]; bw0[c] = up ? mm[c] : bw0[c]; bw1[c] = up ? mn[c] : bw1[c];
    }

    // gap_b
    bool free_row = false, forced = false;
    if constexpr (GENERAL) {
      const bool last_row = (j == lb);
      free_row = last_row && k.no_end;
      forced = k.no_gaps_b && !last_row;
    }
    uint32_t bm[CPL], bn[CPL];
    if (forced) {
#pragma unroll
      for (int c = 0; c < CPL; ++c) { bv[c] = 0; bm[c] = 0u; bn[c] = 0u; }
    } else {
      // max(M, A) of the column to my left, whose it is, and its payload
      const bool la_from_a = av[CPL - 1] >= mv[CPL - 1];
      int zl = wave_shr1(max(mv[CPL - 1], av[CPL - 1]), f.z);
      int zl_a = wave_shr1((int)la_from_a, f.from_a);
      uint32_t zlm = (uint32_t)wave_shr1((int)(la_from_a ? am[CPL - 1] : mm[CPL - 1]), (int)f.zx);
      uint32_t zln = (uint32_t)wave_shr1((int)(la_from_a ? an[CPL - 1] : mn[CPL - 1]), (int)f.zy);
      SpanCand P[CPL];
      const bool floor_pays = !free_row && k.ext > 0;   // only then can the floor of a cell feed a positive cell to its right
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        SpanCand w{free_row ? zl : addw(zl, c1[c]), zl_a, zlm, zln + 1u};   // an opening: its source's pair and the run that begins
        if (floor_pays) {   // the floor of this very cell: it wins a tie with the opening that enters here; a stop, (0, 0),
          // and (0, 1) to the cells that extend out of it: their run begins right of it
          const bool fl = c2[c] >= w.v;
          w = SpanCand{fl ? c2[c] : w.v, fl ? 1 : w.nm, fl ? 0u : w.x, fl ? 1u : w.y};
        }
        if (c == 0) {   // lane 0 continues the previous strip's chain: B(left) + ext, de-trended at g = 0
          const SpanCand carry{free_row ? f.b : addw(addw(f.b, k.ext), trend0), 1, f.bx, f.by + (f.b <= 0 ? 1u : 0u)};   // out of a stop: the run begins here
          const SpanCand wc = span_merge(carry, w);
          const bool l0 = lane == 0;   // (member by member: a select between two structs goes through memory)
          w = SpanCand{l0 ? wc.v : w.v, l0 ? wc.nm : w.nm, l0 ? wc.x : w.x, l0 ? wc.y : w.y};
        }
        P[c] = (c == 0) ? w : span_merge(P[c - 1], w);
        const bool fa_ = av[c] >= mv[c];
        zl = max(mv[c], av[c]); zl_a = fa_;
        zlm = fa_ ? am[c] : mm[c]; zln = fa_ ? an[c] : mn[c];
      }
      const SpanCand incl = wave_scan_span(P[CPL - 1]);
      const SpanCand e{wave_shr1(incl.v, INT32_MIN), 0, (uint32_t)wave_shr1((int)incl.x, 0), (uint32_t)wave_shr1((int)incl.y, 0)};
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const SpanCand pm = span_merge(e, P[c]);
        bv[c] = max(free_row ? pm.v : addw(pm.v, c3[c]), 0);   // (the clamp: the floor is not among the candidates unless it pays)
        bm[c] = bv[c] > 0 ? pm.x : 0u;
        bn[c] = bv[c] > 0 ? pm.y : 0u;
      }
    }

    // the feeds of the next row
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int mb = max(mv[c], bv[c]);
      const bool b_over_m = bv[c] >= mv[c];
      const uint32_t lm = b_over_m ? bm[c] : mm[c], ln = b_over_m ? bn[c] : mn[c];
      const bool d_a = av[c] >= mb, v_a = addw(av[c], k.ext) >= addw(mb, k.open1);
      Da[c] = d_a ? am[c] : lm; Db[c] = d_a ? an[c] : ln;
      Va[c] = v_a ? am[c] : lm; Vb[c] = v_a ? an[c] : ln;
      X[c] = max(av[c], mb);
      if constexpr (GENERAL) Y[c] = mb;
      Ap[c] = av[c];
    }
    if constexpr (!PICK) {
      const bool o_a = av[CPL - 1] >= mv[CPL - 1];
      out.z = max(mv[CPL - 1], av[CPL - 1]); out.b = bv[CPL - 1]; out.from_a = o_a;
      out.zx = o_a ? am[CPL - 1] : mm[CPL - 1]; out.zy = o_a ? an[CPL - 1] : mn[CPL - 1];
      out.bx = bm[CPL - 1]; out.by = bn[CPL - 1];
    } else {
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (c == pick || CPL == 1) {
          const bool o_a = av[c] >= mv[c];
          out.z = max(mv[c], av[c]); out.b = bv[c]; out.from_a = o_a;
          out.zx = o_a ? am[c] : mm[c]; out.zy = o_a ? an[c] : mn[c];
          out.bx = bm[c]; out.by = bn[c];
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

  // SwCountSweep::reduce_best with the two run counts of the winning cell: {score, (column << 32) | row, (gap_runs_a << 32) | gap_runs_b}
  __device__ __forceinline__ void reduce_best(uint32_t col0, int ncol, int &score, unsigned long long &key,
                                              unsigned long long &words) const {
    int b = 0;
    unsigned long long kb = ~0ull, wb = 0;
#pragma unroll
    for (int c = 0; c < CPL; ++c)   // c ascending, strict >: the lowest column wins a tie
      if (c < ncol && bs[c] > b) {
        b = bs[c];
        kb = ((unsigned long long)(col0 + c + 1) << 32) | br[c];
        wb = ((unsigned long long)bw0[c] << 32) | bw1[c];
      }
    score = wave_max_i32(b);
    const unsigned long long mine = (b == score && score > 0) ? kb : ~0ull;
    key = wave_min_u64(mine);
    words = wave_min_u64((mine == key && score > 0) ? wb : ~0ull);   // one lane holds the key
  }
};

// the five results of one pair from the best cell's key and its two run counts, all 0 without a hit
__device__ __forceinline__ void sw_gaps_write(int32_t *score_out, uint32_t *end_a, uint32_t *end_b, uint32_t *gap_runs_a,
                                              uint32_t *gap_runs_b, uint64_t at, int score, unsigned long long key,
                                              unsigned long long words) {
  const bool hit = score > 0;
  score_out[at] = hit ? score : 0;
  end_a[at] = hit ? (uint32_t)(key >> 32) : 0u; end_b[at] = hit ? (uint32_t)key : 0u;
  gap_runs_a[at] = hit ? (uint32_t)(words >> 32) : 0u; gap_runs_b[at] = hit ? (uint32_t)words : 0u;
}

}  // namespace sa
