// sa_score_select.hip -- top-k score search (seqalign_*_score_search): after a tile's score_cross launches, keep the k best
// targets of each query row on the device.
//
// A row of the tile is n_t scores (score_cross_kernel's [q * n_t + t], tile-local target t); the query's running list from
// the earlier target ranges is up to k entries whose targets are all lower than this range's.  An entry's 64-bit key is
// (u << 32) | global_target with u = ~(score ^ 0x80000000): ascending keys are score descending, then target ascending, and
// every key is distinct.  The kernel keeps the k smallest keys of (list ++ row) among the entries with score >= min_score
// (u <= u_max; the list's entries passed that test when they went in) and writes them back sorted.
//
// One workgroup per row, 512 threads.  Over the stream list ++ row (which is in target order):
//   pass 1   count, min u and max u of the passing entries; if count <= k every passing entry is kept;
//   pass 2+  radix select of the k-th smallest u, from the highest bit where min and max differ, up to 11 bits per pass
//            (an LDS histogram of 2 048 bins): SW scores of one row rarely span more than 2 048 values, so one pass;
//   last     compaction: every entry with u < u* is kept, and the first `need` entries with u == u* in stream order -- the
//            lowest targets of the tie group at the cut (ballots, ordered by chunk, load, wave and lane);
//   then a bitonic sort of the <= k kept keys in LDS and the list written back.
// Each pass reads the row's 4-byte scores once (end_a / end_b only for kept entries); loads are 4 per thread in flight.
// The result depends only on the keys, never on the order of LDS atomics.
#include "sa_kernels.h"

namespace {

constexpr int kSelThreads = 512;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelLoads = 4;                        // loads in flight per thread (8: SGPR spills)
constexpr int kSelBits = 11;
constexpr uint32_t kSelBins = 1u << kSelBits;       // 2 048 bins: 4 per thread
constexpr uint32_t kSelMaxK = SEQALIGN_SEARCH_MAX_K;

struct SelShared {
  uint32_t hist[kSelBins];
  unsigned long long key[kSelMaxK];
  uint32_t ea[kSelMaxK], eb[kSelMaxK];
  uint16_t idx[kSelMaxK];
  uint32_t red[3][kSelWaves];                 // per-wave partials: count, min, max (red[0]: the digit scan's too)
  uint32_t wtie[kSelLoads][kSelWaves];        // per (load, wave) tie counts of one chunk
  uint32_t n_sel, digit, below;
};

__device__ __forceinline__ uint32_t key_u(int32_t s) { return ~((uint32_t)s ^ 0x80000000u); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o));
  return v;
}

// f(i, u) for every entry of a part of the stream: the running list (L = 1, u from its keys) or the row (L = kSelLoads
// loads in flight, u from the scores)
template <int L, class U, class F>
__device__ __forceinline__ void each(uint32_t n, uint32_t tid, U get_u, F f) {
  for (uint32_t base = 0; base < n; base += kSelThreads * L) {
    uint32_t u[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const uint32_t i = base + j * kSelThreads + tid;
      u[j] = i < n ? get_u(i) : 0u;
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const uint32_t i = base + j * kSelThreads + tid;
      if (i < n) f(i, u[j]);
    }
  }
}

// the compaction over one part of the stream, chunk by chunk: keep(i, u) for every entry with u < u_star, and for the
// entries with u == u_star whose rank in stream order (tie_base + chunk, load, wave, lane) is below need
template <int L, class U, class F>
__device__ __forceinline__ void compact(SelShared &sh, uint32_t n, uint32_t tid, uint32_t u_max, uint32_t u_star,
                                        uint32_t need, uint32_t &tie_base, U get_u, F keep) {
  const uint32_t lane = tid & 63, wave = tid >> 6;
  for (uint32_t base = 0; base < n; base += kSelThreads * L) {
    uint32_t u[L], rank[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const uint32_t i = base + j * kSelThreads + tid;
      u[j] = i < n ? get_u(i) : ~0u;
    }
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const bool tie = base + j * kSelThreads + tid < n && u[j] <= u_max && u[j] == u_star;
      const unsigned long long m = __ballot(tie);
      rank[j] = __popcll(m & ((1ull << lane) - 1));
      if (lane == 0) sh.wtie[j][wave] = __popcll(m);
    }
    __syncthreads();
    uint32_t chunk_ties = 0;
#pragma unroll
    for (int j = 0; j < L; ++j) {
      uint32_t off = chunk_ties;
#pragma unroll
      for (int w = 0; w < kSelWaves; ++w) {
        off += (uint32_t)w < wave ? sh.wtie[j][w] : 0;
        chunk_ties += sh.wtie[j][w];
      }
      const uint32_t i = base + j * kSelThreads + tid;
      if (i < n && u[j] <= u_max && (u[j] < u_star || (u[j] == u_star && tie_base + off + rank[j] < need))) keep(i, u[j]);
    }
    tie_base += chunk_ties;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kSelThreads) score_select_kernel(SaScoreSelectParams p) {
  __shared__ SelShared sh;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t row_id = blockIdx.x;
  const uint32_t k = p.k, u_max = p.u_max, n_t = p.n_t;
  unsigned long long *lk = p.list_key + row_id * k;
  uint32_t *lea = p.list_ea + row_id * k, *leb = p.list_eb + row_id * k;
  const uint32_t c_old = p.list_n[row_id];
  const int32_t *row = p.score + row_id * n_t;
  const auto old_u = [&](uint32_t i) { return (uint32_t)(lk[i] >> 32); };   // the list's entries passed when they went in
  const auto row_u = [&](uint32_t i) { return key_u(row[i]); };

  // ---- pass 1: count, min, max of the passing entries
  uint32_t cnt = 0, lo = ~0u, hi = 0;
  const auto stat = [&](uint32_t, uint32_t u) {
    if (u <= u_max) { cnt++; lo = min(lo, u); hi = max(hi, u); }
  };
  each<1>(c_old, tid, old_u, stat);
  each<kSelLoads>(n_t, tid, row_u, stat);
  cnt = wave_sum(cnt); lo = wave_min(lo); hi = wave_max(hi);
  if (lane == 0) { sh.red[0][wave] = cnt; sh.red[1][wave] = lo; sh.red[2][wave] = hi; }
  if (tid == 0) sh.n_sel = 0;
  __syncthreads();
  cnt = 0; lo = ~0u; hi = 0;
#pragma unroll
  for (int w = 0; w < kSelWaves; ++w) { cnt += sh.red[0][w]; lo = min(lo, sh.red[1][w]); hi = max(hi, sh.red[2][w]); }
  __syncthreads();

  // ---- the cut: keep u < u_star, and the first `need` entries with u == u_star
  uint32_t u_star = u_max, need = cnt;
  if (cnt > k) {
    uint32_t nb = lo == hi ? 0 : 32 - __clz(lo ^ hi);   // bits below nb differ; above them every passing u equals lo's
    uint32_t prefix = nb >= 32 ? 0u : (uint32_t)(((uint64_t)lo >> nb) << nb);
    uint32_t r = k;                                     // rank (1-based) of the cut among the entries under the prefix
    while (nb > 0) {
      const uint32_t shift = nb > kSelBits ? nb - kSelBits : 0, mask = (1u << (nb - shift)) - 1;
      const uint64_t top = (uint64_t)prefix >> nb;
      for (uint32_t b = tid; b < kSelBins; b += kSelThreads) sh.hist[b] = 0;
      __syncthreads();
      const auto count = [&](uint32_t, uint32_t u) {
        if (u <= u_max && ((uint64_t)u >> nb) == top) atomicAdd(&sh.hist[(u >> shift) & mask], 1u);
      };
      each<1>(c_old, tid, old_u, count);
      each<kSelLoads>(n_t, tid, row_u, count);
      __syncthreads();
      // the digit where the running count reaches r: each thread sums 4 bins, one block-wide exclusive scan
      constexpr uint32_t per = kSelBins / kSelThreads;
      uint32_t part = 0;
#pragma unroll
      for (uint32_t b = 0; b < per; ++b) part += sh.hist[tid * per + b];
      uint32_t incl = part;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= (uint32_t)o) incl += v;
      }
      if (lane == 63) sh.red[0][wave] = incl;
      __syncthreads();
      uint32_t before = 0;
      for (uint32_t w = 0; w < wave; ++w) before += sh.red[0][w];
      const uint32_t excl = before + incl - part;
      if (excl < r && r <= excl + part) {
        uint32_t c = excl;
        for (uint32_t b = 0; b < per; ++b) {
          const uint32_t h = sh.hist[tid * per + b];
          if (c + h >= r) { sh.digit = tid * per + b; sh.below = c; break; }
          c += h;
        }
      }
      __syncthreads();
      prefix |= sh.digit << shift;
      r -= sh.below;
      nb = shift;
      __syncthreads();
    }
    u_star = prefix;
    need = r;
  }

  // ---- compaction: the list first, then the row -- stream order is target order, so the tie group's lowest targets win
  uint32_t tie_base = 0;
  compact<1>(sh, c_old, tid, u_max, u_star, need, tie_base, old_u, [&](uint32_t i, uint32_t) {
    const uint32_t slot = atomicAdd(&sh.n_sel, 1u);
    sh.key[slot] = lk[i]; sh.ea[slot] = lea[i]; sh.eb[slot] = leb[i];
  });
  compact<kSelLoads>(sh, n_t, tid, u_max, u_star, need, tie_base, row_u, [&](uint32_t t, uint32_t u) {
    const uint32_t slot = atomicAdd(&sh.n_sel, 1u);
    const uint64_t at = row_id * n_t + t;
    sh.key[slot] = ((unsigned long long)u << 32) | (p.t_base + t);
    sh.ea[slot] = p.end_a ? p.end_a[at] : 0;
    sh.eb[slot] = p.end_b ? p.end_b[at] : 0;
  });

  // ---- bitonic sort of the kept keys (distinct), padded to a power of two with ~0
  const uint32_t n_sel = sh.n_sel;   // <= k: the cut keeps min(k, cnt)
  uint32_t P = 1;
  while (P < n_sel) P <<= 1;
  for (uint32_t i = tid; i < P; i += kSelThreads) {
    if (i >= n_sel) sh.key[i] = ~0ull;
    sh.idx[i] = (uint16_t)i;
  }
  __syncthreads();
  for (uint32_t size = 2; size <= P; size <<= 1) {
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t t = tid; t < P / 2; t += kSelThreads) {
        const uint32_t a = 2 * t - (t & (stride - 1)), b = a + stride;
        const bool up = (a & size) == 0;
        const unsigned long long ka = sh.key[a], kb = sh.key[b];
        if ((ka > kb) == up) {
          sh.key[a] = kb; sh.key[b] = ka;
          const uint16_t x = sh.idx[a]; sh.idx[a] = sh.idx[b]; sh.idx[b] = x;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < n_sel; i += kSelThreads) {
    lk[i] = sh.key[i];
    lea[i] = sh.ea[sh.idx[i]];
    leb[i] = sh.eb[sh.idx[i]];
  }
  if (tid == 0) p.list_n[row_id] = n_sel;
}

}  // namespace

hipError_t sa_launch_score_select(const SaScoreSelectParams &p, hipStream_t stream) {
  if (p.nq == 0) return hipSuccess;
  if (p.k == 0 || p.k > kSelMaxK || p.n_t == 0) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_SCORE_SELECT, p.nq);
  hipLaunchKernelGGL(score_select_kernel, dim3(p.nq), dim3(kSelThreads), 0, stream, p);
  return hipGetLastError();
}
