// sa_strips.hpp -- the strips pipeline: the pieces shared by the kernels that run the 512-column strips of a wide pair
// as a pipeline of waves (fill_strips_kernel, score_strips_kernel, long_forward_kernel, long_block_kernel).
//
// One workgroup = one wave = one (pair, strip).  The only dependency between strip s and strip s - 1 is the boundary
// column, row by row, so strip s computes its rows in chunks of 64: before a chunk it waits until strip s - 1 has
// published that those rows are done (one uint32 per strip in HBM: strip_publish is an agent-scope release fence and a
// relaxed store, strip_wait a relaxed load in a sleep loop and an acquire fence), then reads its 64 boundary cells.  Strip
// s therefore runs 64 rows behind s - 1: a pair with S strips takes len_b + 64 * S row steps instead of len_b * S.
//
// Why the waits are safe under any dispatch order.  A workgroup does NOT take its strip from blockIdx: it draws a TICKET
// from an atomic counter when it starts running (strip_ticket; the counter sits behind the progress words), and a ticket
// decodes strip-major (strip_of_ticket: group of 8 pairs, strip, pair in group; the one-pair kernels use the ticket as the
// strip).  A strip's ticket is therefore always higher than the ticket of the strip it waits for, and a ticket only
// exists once its workgroup is resident on a CU -- so a waiting wave only ever waits for waves that are running or
// finished, whatever order the hardware dispatches workgroups in (other contexts' kernels, CU masks, preemption).  No
// cooperative launch, no dispatch-order assumption, no watchdog.  Tickets are drawn roughly in dispatch order, so one
// pair's strips (8 tickets apart) still tend to land on one XCD.
//
// What strip s hands strip s + 1 differs.  The kernels that store the matrices read the left strip's last column back
// from them (RowFeed, sa_rowsweep.hpp).  The score kernels store nothing per cell and hand over a scratch column instead
// (StripHandoff below); SW adds the best cell so far (BestCells, merge_left_best).  The span kernel (sa_span.hip) hands over
// the same column with the spans of its two values (StripSpanHandoff, merge_left_best_span): same waits, same publishes.
#pragma once

#include "sa_rowsweep.hpp"

namespace sa {

__device__ __forceinline__ uint32_t strip_ticket(uint32_t *counter) {
  uint32_t t = 0;
  if (threadIdx.x == 0) t = atomicAdd(counter, 1u);
  return __builtin_amdgcn_readfirstlane(t);
}

// the batch form: ticket = (group * strips_per_pair + strip) * 8 + pair_in_group
__device__ __forceinline__ void strip_of_ticket(uint32_t ticket, uint32_t strips_per_pair, uint32_t &strip, uint32_t &pair) {
  const uint32_t in_group = ticket & 7u, gs = ticket >> 3;
  strip = gs % strips_per_pair;
  pair = (gs / strips_per_pair) * 8 + in_group;
}

// (the strip that owns `word` holds a lower ticket: it is resident or done)
__device__ __forceinline__ void strip_wait(const uint32_t *word, uint32_t need) {
  while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) __builtin_amdgcn_s_sleep(8);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the boundary loads that follow see those rows
}

__device__ __forceinline__ void strip_publish(uint32_t *word, uint32_t value) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  if (threadIdx.x == 0) __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The hand-off column of the score kernels: per row, max(M, A) and B of a strip's last column (RowSweep::row's feedZ /
// feedB; the up-left boundX follows from them), 8 bytes into a scratch column of len_b + 1 rows per strip.  Moved 64 rows
// at a time: lane q holds row j0 + q's values, the 64 rows leave as one coalesced 512-byte store.
struct StripHandoff {
  int code = 0, fz = 0, fb = 0;   // lane q: row j0 + q's code and, from the strip to my left, max(M, A) and B
  int oz = 0, ob = 0;             // lane q: row j0 + q's values of my last column, for the strip to my right

  // every 64 rows, after the wait: this lane's row r = j0 + lane
  __device__ __forceinline__ void load(const SaFillParams &p, const SweepConsts &k, const Border &bd,
                                       const uint8_t *__restrict__ seq_b, uint32_t lb, uint32_t strip,
                                       const int32_t *hand_in, uint32_t r) {
    if (r <= lb) {
      code = p.code[seq_b[r - 1]];
      if (strip == 0) {   // border column (reference alignment.c:72-80)
        fz = max(k.floor_, bd.edge_gap(r));
        fb = k.floor_;
      } else {
        const int2 h = *reinterpret_cast<const int2 *>(hand_in + 2ull * r);
        fz = h.x; fb = h.y;
      }
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);   // once per 64 rows (see RowFeed::load)
  }

  // every row of a strip that is not the last (such a strip is full: lane 63's last column is the strip's); publishes
  // the rows it stores to `word`, except the last ones: those wait for the best cell
  template <int CPL>
  __device__ __forceinline__ void keep(const int (&mv)[CPL], const int (&av)[CPL], const int (&bv)[CPL], int32_t *hand_out,
                                       uint32_t *word, int lane, int q, uint32_t j, uint32_t lb) {
    const int z = read_lane(max(mv[CPL - 1], av[CPL - 1]), kWave - 1), b = read_lane(bv[CPL - 1], kWave - 1);
    oz = (lane == q) ? z : oz;
    ob = (lane == q) ? b : ob;
    if (q == kWave - 1 || j == lb) {
      if (lane <= q) *reinterpret_cast<int2 *>(hand_out + 2ull * (j - q + lane)) = make_int2(oz, ob);
      if (j != lb) strip_publish(word, j);
    }
  }
};

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// per-column running best of match_scores (SW)
template <int CPL>
struct BestCells {
  int s[CPL];
  uint32_t r[CPL];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int c = 0; c < CPL; ++c) { s[c] = 0; r[c] = 0; }
  }
  __device__ __forceinline__ void row(const int (&mv)[CPL], uint32_t j) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool up = mv[c] > s[c];   // strict: the first (lowest) row keeps a tie
      s[c] = up ? mv[c] : s[c];
      r[c] = up ? j : r[c];
    }
  }
  // the wave's best in hit order over my columns col0 + 1 .. (matrix column = col0 + c + 1): {score, (column << 32) | row};
  // score 0 -> key ~0
  __device__ __forceinline__ void reduce(uint32_t col0, int ncol, int &score, unsigned long long &key) const {
    int b = 0;
    unsigned long long kb = ~0ull;
#pragma unroll
    for (int c = 0; c < CPL; ++c)   // c ascending, strict >: the lowest column wins a tie
      if (c < ncol && s[c] > b) { b = s[c]; kb = ((unsigned long long)(col0 + c + 1) << 32) | r[c]; }
    score = wave_max_i32(b);
    key = wave_min_u64(b == score && score > 0 ? kb : ~0ull);
  }
};

// strip_best: per strip that is not the last, {score, end_a, end_b, 0} of the best cell of strips 0 .. s.  Strip s merges
// the entry of the strip to its left (visible: it waited for that strip's last rows, and the entry was written before
// they were published) into its own best and hands that on; the last strip's is the pair's.
__device__ __forceinline__ void merge_left_best(const uint32_t *left_entry, int &score, unsigned long long &key) {
  const uint4 left = *reinterpret_cast<const uint4 *>(left_entry);
  if ((int)left.x >= score && (int)left.x > 0) {   // a tie goes to the lower column: theirs
    score = (int)left.x;
    key = ((unsigned long long)left.y << 32) | left.z;
  }
}

// ---- the span kernel's forms (sa_span.hip) ----
constexpr int kSpanHandoffInts = SA_SPAN_HANDOFF_BYTES / 4;   // per row of a hand-off column
constexpr int kSpanBestWords = SA_SPAN_BEST_BYTES / 4;        // per strip_best entry

// StripHandoff with spans: per row {max(M, A), B, whether max(M, A) is A's, 0} and {span of that state, span of B} of a
// strip's last column, 32 bytes.  Moved 64 rows at a time: lane q holds row j0 + q, the 64 rows leave as 2 KiB in a row.
struct StripSpanHandoff {
  int code = 0;
  int4 in0 = {0, 0, 0, 0}, in1 = {0, 0, 0, 0};     // lane q: row j0 + q, from the strip to my left
  int4 out0 = {0, 0, 0, 0}, out1 = {0, 0, 0, 0};   // lane q: row j0 + q of my last column

  // every 64 rows, after the wait: this lane's row r = j0 + lane; i0 = the column left of the strip
  __device__ __forceinline__ void load(const SaFillParams &p, const uint8_t *__restrict__ seq_b, uint32_t lb, uint32_t strip,
                                       uint32_t i0, const int32_t *hand_in, uint32_t r) {
    if (r <= lb) {
      code = p.code[seq_b[r - 1]];
      if (strip == 0) {   // the border column holds 0: a walk that reaches (0, r) stops there
        in0 = make_int4(0, 0, 0, 0);
        in1 = make_int4((int)i0, (int)r, (int)i0, (int)r);
      } else {
        const int4 *h = reinterpret_cast<const int4 *>(hand_in + (uint64_t)kSpanHandoffInts * r);
        in0 = h[0]; in1 = h[1];
      }
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);   // once per 64 rows (see RowFeed::load)
  }

  // every row of a strip that is not the last; o0 / o1: the row's entry (wave-uniform).  Publishes the rows it stores to
  // `word`, except the last ones: those wait for the best cell
  __device__ __forceinline__ void keep(const int4 &o0, const int4 &o1, int32_t *hand_out, uint32_t *word, int lane, int q,
                                       uint32_t j, uint32_t lb) {
    const bool mine = lane == q;   // (member by member: a select between two vectors may go through memory)
    out0 = make_int4(mine ? o0.x : out0.x, mine ? o0.y : out0.y, mine ? o0.z : out0.z, 0);
    out1 = make_int4(mine ? o1.x : out1.x, mine ? o1.y : out1.y, mine ? o1.z : out1.z, mine ? o1.w : out1.w);
    if (q == kWave - 1 || j == lb) {
      if (lane <= q) {
        int4 *h = reinterpret_cast<int4 *>(hand_out + (uint64_t)kSpanHandoffInts * (j - q + lane));
        h[0] = out0; h[1] = out1;
      }
      if (j != lb) strip_publish(word, j);
    }
  }
};

// merge_left_best with the span of the best cell: an entry is {score, end_a, end_b, 0} {pos_a, pos_b, 0, 0}
__device__ __forceinline__ void merge_left_best_span(const uint32_t *left_entry, int &score, unsigned long long &key,
                                                     unsigned long long &span) {
  const uint4 left = reinterpret_cast<const uint4 *>(left_entry)[0], lspan = reinterpret_cast<const uint4 *>(left_entry)[1];
  if ((int)left.x >= score && (int)left.x > 0) {   // a tie goes to the lower column: theirs
    score = (int)left.x;
    key = ((unsigned long long)left.y << 32) | left.z;
    span = ((unsigned long long)lspan.x << 32) | lspan.y;
  }
}

}  // namespace sa
