// sa_payload_kernels.hpp -- the kernel shell of the payload sweeps: the families that carry two payload words beside each state
// of a cell through sa_score.hip's row sweep (sa_span.hip, sa_nw_stats.hip, sa_sw_stats.hip).  DESIGN.md 3.23.
//   payload_rows_kernel    rows of up to SA_SPAN_ROW_MAX columns, one wave per pair (1 .. 6 or 8 columns per lane), 4 pairs per
//                          workgroup; its CROSS form takes a query and a target of two sets instead of a pair of a list
//   payload_strips_kernel  wider rows, the strips pipeline of sa_strips.hpp with StripSpanHandoff's 32 bytes per row and strip
//   launch_payload_*       their ladders over the columns per lane and the scoring, recorded as "score_rows" / "score_cross" /
//                          "score_strips"
// A family is a policy F: types and static device functions, no state, nothing decided at run time.  It names
//   Params                          the family's parameter block (sa_kernels.h)
//   Sweep<CPL, SUBST, GENERAL>      its sweep; row, reduce_err and what the ends below call are the sweep's own
//   border(p)                       what the two border functions need of the scoring (NoBorder: nothing)
//   start_strip(sw, p, k, bd, ...)  the sweep's start_strip
//   border_feed(k, bd, j)           the rows kernel's feed of row j: cell (0, j) of the border column
//   strip0_feed(h, k, bd, r)        the same cell in hand-off form, over what strip 0 loaded for its row r
//   kBestCell                       what the result is taken from.  true (SW): the best cell in hit order with its two payload
//                                   words, sw.reduce_best -- a strip merges its own into the best of the strips to its left
//                                   (merge_left_best_span) and hands that on, and write(sp, at, score, key, words) turns the
//                                   cell into the family's result words.  false (NW): the cell (len_a, len_b), sw.write by
//                                   the lane that owns it, nothing but the rows goes from strip to strip, and
//                                   write_border(sp, k, bd, at, lb) is the result of a pair without columns
// Included by a family's .hip file after its sweep's header.
#pragma once
#include "sa_span.hpp"   // SpanFeed, the strips' width; sa_strips.hpp

namespace sa {

struct NoBorder {};   // SW: the border column holds zeros

// CROSS (kind "score_cross"): sa_score.hip's CROSS form -- wave w of a launch for one row class takes target t_order[w / nq]
// and query q_list[w % nq], longest targets first, writes its result words at [q * n_t + t] of the tile and leaves a failing
// pair's tile-local index in one 64-bit atomicMin.  Same sweep, same picks.
template <class F, int CPL, int SUBST, bool GENERAL, bool CROSS = false>
__global__ void __launch_bounds__(kWave *kWavesPerBlock)
payload_rows_kernel(const std::conditional_t<CROSS, SaCrossParams<typename F::Params>, typename F::Params> kp) {
  const typename F::Params &sp = sa_pair_params(kp);
  const SaFillParams &p = sp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t pair = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  uint32_t qa = pair, tb = pair;   // descriptors of seq_a and seq_b
  uint64_t at = pair;              // where the result goes
  if constexpr (CROSS) {
    if (pair >= kp.n_waves) return;   // wave-uniform, after the only barrier
    const uint32_t ti = pair / kp.nq;
    qa = kp.q_list[pair - ti * kp.nq];
    tb = kp.t_order[ti];
    at = (uint64_t)qa * kp.n_t + tb;
  } else {
    if (pair >= p.n_pairs) return;   // wave-uniform, after the only barrier
  }

  const uint32_t la = p.len_a[qa], lb = p.len_b[tb];
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[qa];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[tb];
  const uint32_t W = la + 1;
  const SweepConsts k(p, table);
  const auto bd = F::border(p);

  typename F::template Sweep<CPL, SUBST, GENERAL> sw;
  const uint32_t col0 = lane * CPL;
  const int ncol = max(0, min(CPL, (int)la - lane * CPL));
  F::start_strip(sw, p, k, bd, sa_, la, 0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)

  int code = 0;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {   // every 64 rows: lane t fetches seq_b's code for row j + t
      const uint32_t r = j + lane;
      if (r <= lb) code = p.code[sb_[r - 1]];
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
    }
    const SpanFeed f = F::border_feed(k, bd, j);
    SpanFeed out;
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code, q), f, out);
  }

  const unsigned long long err = sw.reduce_err();
  int score;
  unsigned long long key, words;   // kBestCell: the best cell, written by lane 0 below
  if constexpr (F::kBestCell) {
    sw.reduce_best(col0, ncol, score, key, words);
  } else if (la == 0) {   // cell (0, len_b) of the border column
    if (lane == 0) F::write_border(sp, k, bd, at, lb);
  } else {
    sw.write(sp, at, col0, la);
  }
  if (lane == 0) {
    if constexpr (F::kBestCell) F::write(sp, at, score, key, words);
    if constexpr (CROSS) {
      if (err != ~0ull) {
        atomicMin(kp.err_pair, (unsigned long long)at);
        atomicOr(sp.err_flag, 1u);
      }
    } else {
      p.status[pair] = err;
      if (err != ~0ull) atomicOr(sp.err_flag, 1u);
    }
  }
}

template <class F, int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave)
payload_strips_kernel(const typename F::Params sp) {
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
  const auto bd = F::border(p);
  const uint32_t cols = (i0 < la) ? min(kSpanStripCols, la - i0) : 0;
  const bool last_strip = i0 + kSpanStripCols >= la;
  const uint32_t col0 = i0 + lane * CPL;
  const int ncol = max(0, min(CPL, (int)cols - lane * CPL));
  typename F::template Sweep<CPL, SUBST, GENERAL> sw;
  F::start_strip(sw, p, k, bd, sa_, la, i0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);

  StripSpanHandoff h;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {
      // rows j .. j + 63 of the strip to my left must have been handed over
      if (strip > 0) strip_wait(done + strip - 1, min(j + kWave - 1, lb));
      h.load(p, sb_, lb, strip, i0, hand_in, j + lane);
      if (strip == 0) F::strip0_feed(h, k, bd, j + lane);   // the border column in place of what a strip hands over
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
  if constexpr (F::kBestCell) {
    int score;
    unsigned long long key, words;
    sw.reduce_best(col0, ncol, score, key, words);
    if (strip > 0 && lb > 0) merge_left_best_span(sp.strip_best + kSpanBestWords * (slot - 1), score, key, words);
    if (lane == 0) {
      if (last_strip) {
        F::write(sp, pair, score, key, words);
      } else {
        uint4 *entry = reinterpret_cast<uint4 *>(sp.strip_best + kSpanBestWords * slot);
        entry[0] = make_uint4((uint32_t)score, (uint32_t)(key >> 32), (uint32_t)key, 0u);
        entry[1] = make_uint4((uint32_t)(words >> 32), (uint32_t)words, 0u, 0u);
      }
    }
  }
  if (last_strip) {
    if constexpr (!F::kBestCell) sw.write(sp, pair, col0, la);
  } else if (lb > 0) {
    strip_publish(done + strip, lb);   // the last rows (and the best cell so far)
  }
}

template <class P> inline uint32_t one_wave_waves(const P &p) { return p.f.n_pairs; }
template <class P> inline uint32_t one_wave_waves(const SaCrossParams<P> &p) { return p.n_waves; }

// the columns per lane of the widest row (sa_span_row_class's steps), then the scoring
template <class F, bool CROSS, class P>
hipError_t launch_payload_one_wave(const P &p, uint32_t max_len_a, hipStream_t stream) {
  return launch_by_cpl<1, 2, 3, 4, 5, 6, 8>(columns_per_lane(max_len_a), [&](auto cpl) {
    const dim3 grid((one_wave_waves(p) + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
    launch_by_scoring(sa_pair_params(p).f, [&](auto subst, auto general, uint32_t table_ints) {
      hipLaunchKernelGGL((payload_rows_kernel<F, decltype(cpl)::value, subst(), general(), CROSS>), grid, block, table_ints * sizeof(int32_t), stream, p);
    });
    return hipGetLastError();
  });
}

// every pair of the launch has len_a <= SA_SPAN_ROW_MAX; max_len_a picks the columns per lane
template <class F>
hipError_t launch_payload_rows(const typename F::Params &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_ROWS, p.f.n_pairs);
  return launch_payload_one_wave<F, false>(p, max_len_a, stream);
}

// every query of the class has len_a <= max_len_a <= SA_SPAN_ROW_MAX
template <class F>
hipError_t launch_payload_cross(const SaCrossParams<typename F::Params> &p, uint32_t max_len_a, hipStream_t stream) {
  if (p.n_waves == 0) return hipSuccess;
  if (max_len_a > SA_SPAN_ROW_MAX || p.nq == 0) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_CROSS, p.n_waves);
  return launch_payload_one_wave<F, true>(p, max_len_a, stream);
}

// the caller zeroed progress (and err_flag) and set status to ~0
template <class F>
hipError_t launch_payload_strips(const typename F::Params &p, hipStream_t stream) {
  if (p.f.n_pairs == 0) return hipSuccess;
  const uint64_t blocks = (uint64_t)((p.f.n_pairs + 7) / 8) * 8 * p.strips_per_pair;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_STRIPS, p.f.n_pairs);
  launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((payload_strips_kernel<F, subst(), general()>), dim3((unsigned)blocks), dim3(kWave),
                       table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa
