// sa_nw_gaps.hpp -- the arithmetic of the NW gap-run sweeps (sa_nw_gaps.hip, sa_band_nw_gaps.hip): NwGapSweep, one matrix row per
// step, StatSweep's NW values, admission tests, marks and selections (sa_nw_stats.hpp) with another meaning in the two payload
// words beside each of match, gap_a and gap_b:
//   word 0  x = gap_runs_a    the maximal runs of gap_a columns ('-' in string a) of the walk that starts in that state,
//   word 1  y = gap_runs_b    its maximal runs of gap_b columns ('-' in string b); bit 31 is the sticky mark "no walk starts
//                             here" (SA_STATS_NO_WALK).
// A walk has fewer than len_a + len_b < 2^31 columns, so neither count reaches bit 31 at any length and adding one never clears
// the mark.  A run is counted at its FIRST column in forward order, which is the last gap state the walk passes before it leaves
// the run: a gap state adds one unless the predecessor the walker picks is the same gap state in a cell that is not on the
// border.  A walk that reaches the border leaves the loop there and the rest is ONE run of gap columns: a cell (x, 0), x > 0,
// holds (0, 1), a cell (0, y), y > 0, holds (1, 0) and (0, 0) holds (0, 0), whatever the state.  Every feed and hand-off stays
// in RAW form (the pair of the state it names); the increment is decided in the consuming cell, as in SwGapSweep:
//   gap_a   + 1 in x unless the extension wins the vertical feed and the row above is not row 0 (under a_free the test is the
//           diagonal pick's: gap_a above holds the maximum);
//   gap_b   every opening candidate of the row scan carries its source's pair + 1 in y; the chain carried in from the left
//           strip does not add, the border column's does (the cell left of column 1 is on the border).
// The match state adds nothing.  The scan's element, its merge and the feed of a strip are sa_span.hpp's: in a SpanCand /
// SpanFeed here x is word 0 and y word 1.  The definition is in sa_nw_gaps.hip's header.
#pragma once
#include "sa_span.hpp"

namespace sa {

template <int CPL, int SUBST, bool GENERAL>
struct NwGapSweep {
  int fa[CPL], arow[CPL];
  int X[CPL], Ap[CPL];
  int Y[GENERAL ? CPL : 1];
  int c1[CPL], c2[CPL], c3[CPL];
  // previous row: the diagonal and the vertical feed, {gap_runs_a, gap_runs_b | mark} each -- by StatSweep's names (m: word 0,
  // n: word 1), which the NW band frame reads (sa_band_nw_frame.hpp)
  uint32_t Dm[CPL], Dn[CPL], Vm[CPL], Vn[CPL];
  int boundX;                                    // max3 of the cell left of the strip on the previous row ...
  uint32_t boundDm, boundDn;                     // ... and its diagonal feed
  int trend0;
  unsigned long long err = ~0ull;

  // StatSweep::start_strip; row 0 is the border: cell (x, 0), x > 0, is one run of gap_b columns, cell (0, 0) none
  __device__ __forceinline__ void start_strip(const SaFillParams &p, const SweepConsts &k, const Border &bd,
                                              const uint8_t *__restrict__ seq_a, uint32_t la, uint32_t i0, uint32_t col0, int lane) {
    trend0 = k.ext > 0 ? mulw(kWave * CPL, k.ext) : 0;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const uint32_t idx = col0 + c;
      const int code = idx < la ? (int)p.code[seq_a[idx]] : 0;
      fa[c] = code & 0xff;
      arow[c] = (code >> 8) * k.K;
      const int b0 = bd.edge_gap(idx + 1);
      X[c] = max(k.floor_, b0);
      if constexpr (GENERAL) Y[c] = max(k.floor_, b0);
      Ap[c] = k.floor_;
      Dm[c] = Vm[c] = 0u; Dn[c] = Vn[c] = 1u;
      const int g_ext = subw(mulw(lane * CPL + c, k.ext), trend0);   // -t(g)
      c1[c] = subw(k.open1, g_ext);
      c2[c] = subw(k.floor_, g_ext);
      c3[c] = g_ext;
    }
    boundX = (i0 == 0) ? 0 : max(k.floor_, bd.edge_gap(i0));
    boundDm = 0u; boundDn = (i0 == 0) ? 0u : 1u;   // the up-left of the strip's first column on row 1: cell (i0, 0)
  }

  // Row j.  f: the cell left of the strip on this row.  Leaves the last column's hand-off in `out` (lane 63's is the strip's).
  // PICK (band_nw_payload_strips_kernel, where the strip's last column moves through the frame): `out` is column `pick` of the
  // lane instead of its last.
  template <bool PICK = false>
  __device__ __forceinline__ void row(const SweepConsts &k, uint32_t j, uint32_t lb, uint32_t la, uint32_t W, int lane,
                                      uint32_t col0, int ncol, int code_b, const SpanFeed &f, SpanFeed &out, int pick = CPL - 1) {
    bool free_row = false, forced = false;   // wave-uniform: gap_b of this row costs nothing / is not admitted
    if constexpr (GENERAL) {
      const bool last_row = (j == lb);
      free_row = last_row && k.no_end;
      forced = k.no_gaps_b && !last_row;
    }
    const bool above_inner = j > 1;   // wave-uniform: the row above is not the border row
    int xd = wave_shr1(X[CPL - 1], boundX);
    uint32_t dm = (uint32_t)wave_shr1((int)Dm[CPL - 1], (int)boundDm), dn = (uint32_t)wave_shr1((int)Dn[CPL - 1], (int)boundDn);
    {   // the boundary cell of this row, for the next one: A > B > M over {max(M, A) and whose it is, B}
      boundX = max(f.z, f.b);
      const bool zwins = forced || (f.from_a ? f.z >= f.b : f.z > f.b);
      boundDm = zwins ? f.zx : f.bx;
      boundDn = zwins ? f.zy : f.by;
    }
    int mv[CPL], av[CPL], bv[CPL];
    uint32_t mm[CPL], mn[CPL], am[CPL], an[CPL];
    bool a_adm[CPL];   // gap_a of this column is admitted as a predecessor (and can be walked into)
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int s = subst_score<SUBST>(fa[c], arow[c], code_b, k.table, k.gen_eq, k.gen_ne);
      const int m_raw = addw(xd, s);
      int m, a, a_raw;
      bool walk_m = m_raw >= k.floor_, a_free = false;   // a state clamped with every candidate below the floor has no walk
      bool a_ext;                                        // the extension wins gap_a's two candidates (the V feed's own test)
      a_adm[c] = true;
      if constexpr (GENERAL) {
        m = max(m_raw, k.floor_);
        if (s == SA_S_BLOCKED || s == SA_S_UNKNOWN) {
          m = k.floor_;
          walk_m = false;
          if (s == SA_S_UNKNOWN && c < ncol) err = min(err, (unsigned long long)j * W + col0 + c + 1);
        }
        const bool last_col = (col0 + c + 1 == la);
        a_free = last_col && k.no_end;   // max3 of the cell above, no penalty: its diagonal feed is this state's too
        a_adm[c] = !k.no_gaps_a || last_col;
        const int a_open = addw(Y[c], k.open1), a_cont = addw(Ap[c], k.ext);
        a_raw = max(a_open, a_cont);
        a = a_free ? max(Y[c], Ap[c]) : a_adm[c] ? max(a_raw, k.floor_) : k.floor_;
        a_ext = a_free ? Ap[c] >= Y[c] : a_cont >= a_open;
      } else {
        m = max(m_raw, k.floor_);
        const int a_open = addw(X[c], k.open1), a_cont = addw(Ap[c], k.ext);   // (open1 <= ext: RowSweep::row)
        a_raw = max(a_open, a_cont);
        a = max(a_raw, k.floor_);
        a_ext = a_cont >= a_open;
      }
      // the match state adds nothing; gap_a opens a run here unless it extends the gap_a of a cell above that is not on the border
      const uint32_t a_inc = (a_ext && above_inner) ? 0u : 1u;
      mm[c] = walk_m ? dm : 0u;
      mn[c] = walk_m ? dn : SA_STATS_NO_WALK;
      const bool walk_a = a_free || (a_adm[c] && a_raw >= k.floor_);
      am[c] = walk_a ? (a_free ? Dm[c] : Vm[c]) + a_inc : 0u;
      an[c] = walk_a ? (a_free ? Dn[c] : Vn[c]) : SA_STATS_NO_WALK;
      xd = X[c]; dm = Dm[c]; dn = Dn[c];
      mv[c] = m; av[c] = a;
    }

    // gap_b
    uint32_t bm[CPL], bn[CPL];
    if (forced) {
#pragma unroll
      for (int c = 0; c < CPL; ++c) { bv[c] = k.floor_; bm[c] = 0u; bn[c] = SA_STATS_NO_WALK; }
    } else {
      // max(M, A) of the column to my left, whether it is an admitted A's, and its payload
      const bool la_from_a = a_adm[CPL - 1] && av[CPL - 1] >= mv[CPL - 1];
      int zl = wave_shr1(max(mv[CPL - 1], av[CPL - 1]), f.z);
      int zl_a = wave_shr1((int)la_from_a, f.from_a);
      uint32_t zlm = (uint32_t)wave_shr1((int)(la_from_a ? am[CPL - 1] : mm[CPL - 1]), (int)f.zx);
      uint32_t zln = (uint32_t)wave_shr1((int)(la_from_a ? an[CPL - 1] : mn[CPL - 1]), (int)f.zy);
      SpanCand P[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        SpanCand w{free_row ? zl : addw(zl, c1[c]), zl_a, zlm, zln + 1u};   // an opening: its source's pair and the run that begins
        if (!free_row) {   // the floor of this very cell: it loses a tie to every candidate, and no walk starts in it
          const bool fl = c2[c] > w.v;
          w = SpanCand{fl ? c2[c] : w.v, fl ? 0 : w.nm, fl ? 0u : w.x, fl ? SA_STATS_NO_WALK : w.y};
        }
        if (c == 0) {   // lane 0 continues the previous strip's chain: B(left) + ext, de-trended at g = 0; out of the border
          // column (the cell left of column 1) the run begins here
          const SpanCand carry{free_row ? f.b : addw(addw(f.b, k.ext), trend0), 1, f.bx, f.by + (col0 == 0 ? 1u : 0u)};
          const SpanCand wc = span_merge(carry, w);
          const bool l0 = lane == 0;   // (member by member: a select between two structs goes through memory)
          w = SpanCand{l0 ? wc.v : w.v, l0 ? wc.nm : w.nm, l0 ? wc.x : w.x, l0 ? wc.y : w.y};
        }
        P[c] = (c == 0) ? w : span_merge(P[c - 1], w);
        const bool fa_ = a_adm[c] && av[c] >= mv[c];
        zl = max(mv[c], av[c]); zl_a = fa_;
        zlm = fa_ ? am[c] : mm[c]; zln = fa_ ? an[c] : mn[c];
      }
      const SpanCand incl = wave_scan_span(P[CPL - 1]);
      const SpanCand e{wave_shr1(incl.v, INT32_MIN), 0, (uint32_t)wave_shr1((int)incl.x, 0), (uint32_t)wave_shr1((int)incl.y, 0)};
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const SpanCand pm = span_merge(e, P[c]);
        bv[c] = free_row ? pm.v : addw(pm.v, c3[c]);   // (the floor is among the candidates: no clamp)
        bm[c] = pm.x; bn[c] = pm.y;
      }
    }

    // the feeds of the next row: the first of A, B, M (admitted) that holds the maximum / the largest candidate of gap_a below
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int mb = max(mv[c], bv[c]);
      const bool b_over_m = !forced && bv[c] >= mv[c];
      const uint32_t lm = b_over_m ? bm[c] : mm[c], ln = b_over_m ? bn[c] : mn[c];
      const bool d_a = a_adm[c] && av[c] >= mb, v_a = addw(av[c], k.ext) >= addw(mb, k.open1);
      Dm[c] = d_a ? am[c] : lm; Dn[c] = d_a ? an[c] : ln;
      Vm[c] = v_a ? am[c] : lm; Vn[c] = v_a ? an[c] : ln;
      X[c] = max(av[c], mb);
      if constexpr (GENERAL) Y[c] = mb;
      Ap[c] = av[c];
    }
    if constexpr (!PICK) {
      const bool o_a = a_adm[CPL - 1] && av[CPL - 1] >= mv[CPL - 1];
      out.z = max(mv[CPL - 1], av[CPL - 1]); out.b = bv[CPL - 1]; out.from_a = o_a;
      out.zx = o_a ? am[CPL - 1] : mm[CPL - 1]; out.zy = o_a ? an[CPL - 1] : mn[CPL - 1];
      out.bx = bm[CPL - 1]; out.by = bn[CPL - 1];
    } else {
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (c == pick || CPL == 1) {
          const bool o_a = a_adm[c] && av[c] >= mv[c];
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

  // After the last row, from the lane that owns column len_a: X is the score, and the diagonal feed of that cell is the end
  // pick's pair, raw (StatSweep::write).  SaNwGapsParams: matches is gap_runs_a, mismatches gap_runs_b
  __device__ __forceinline__ void write(const SaStatsParams &sp, uint64_t at, uint32_t col0, uint32_t la) const {
#pragma unroll
    for (int c = 0; c < CPL; ++c)
      if (col0 + c + 1 == la) { sp.score[at] = X[c]; sp.matches[at] = Dm[c]; sp.mismatches[at] = Dn[c]; }
  }
};

}  // namespace sa
