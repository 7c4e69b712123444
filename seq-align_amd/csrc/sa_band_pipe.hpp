// sa_band_pipe.hpp -- the pieces every banded kernel shares, written once: the frame's shift (wave_shl1, frame_shift) and
// the banded SW best cell (BandBest) of the one-wave kernels (sa_band.hip, sa_band_frame.hpp, sa_band_nw_stats.hip) and of
// the wide ones, and the wide pipeline's own: the publication that counts in the pair's front word (band_publish), the
// bounded wait (band_strip_wait), the way out of a wait that ran dry (band_give_up) and the launch side (band_strips_grid,
// launch_by_strip_cols).  The wide kernels are band_strips_kernel (sa_band_strips.hip), band_nw_stats_strips_kernel
// (sa_band_nw_stats_strips.hip) and band_payload_strips_kernel (sa_band_frame.hpp).  DESIGN.md 3.29.
//
// The wait.  band_strip_wait is the wide kernels' own and is bounded.  Its budget, kBandWaitTicks of the 100 MHz wall clock,
// restarts whenever the awaited word advances; when it runs out the wave looks at the pair's FRONT word, which every strip
// of the pair bumps with each publication (a strip far right of the pipeline's front watches a word that stays 0 until
// the front arrives, but the front word moves all the while), and restarts the budget if that has moved since the budget
// started.  Only when no strip of the pair has published for a whole budget -- some running strip publishes every 64 row
// steps, so only preemption stretches that -- does it give up: it records its pair in the give-up
// word (the first to give up stays) and publishes ~0 itself so that the strips to its right fall through; the host then
// fails the call (SEQALIGN_E_HIP, "band strip hand-off timed out", that pair named).
#pragma once
#include <type_traits>

#include "sa_strips.hpp"

namespace sa {

constexpr unsigned long long kBandWaitTicks = 200000000ull;   // 2 s of the 100 MHz wall clock
constexpr uint32_t kAllRows = 0xFFFFFFFFu;                     // a progress word: "all my rows"

// Full-wave shift left by one lane: lane l receives src of lane l + 1, lane 63 receives lane63_value.  DPP ctrl 0x130 =
// wave_shl:1, the mirror of wave_shr1 (sa_fill_common.hpp).
__device__ __forceinline__ int wave_shl1(int src, int lane63_value) {
  return __builtin_amdgcn_update_dpp(lane63_value, src, 0x130, 0xf, 0xf, false);
}

// the frame moves one column to the right: every position takes its right neighbour's value, the last one `enters`; for the
// sweeps' int and uint32_t arrays
template <class T, int N>
__device__ __forceinline__ void frame_shift(T (&a)[N], T enters) {
  const T first = a[0];
#pragma unroll
  for (int c = 0; c + 1 < N; ++c) a[c] = a[c + 1];
  a[N - 1] = (T)wave_shl1((int)first, (int)enters);
}

// banded SW: the running best of match_scores per frame position, and of the columns that have left the frame
template <int CPL>
struct BandBest {
  int s[CPL], r[CPL];                     // of the column each of my positions holds: best value, first row that reached it
  int ret_s = 0, ret_col = 0, ret_row = 0;   // of the columns left of the frame (wave-uniform)
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int c = 0; c < CPL; ++c) { s[c] = 0; r[c] = 0; }
  }
  // the frame moves off column `col`: it retires (a tie stays with the retired, lower columns), the others shift with the frame
  __device__ __forceinline__ void retire(int col) {
    const int s0 = read_lane(s[0], 0), r0 = read_lane(r[0], 0);
    if (s0 > ret_s) { ret_s = s0; ret_col = col; ret_row = r0; }
    frame_shift(s, 0);
    frame_shift(r, 0);
  }
  __device__ __forceinline__ void row(const int (&mv)[CPL], uint32_t j, int ncol) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool up = c < ncol && mv[c] > s[c];   // strict: the first (lowest) row keeps a tie
      s[c] = up ? mv[c] : s[c];
      r[c] = up ? (int)j : r[c];
    }
  }
  // the pair's best in hit order; my position c holds column col0 + c.  score 0: key ~0
  __device__ __forceinline__ void reduce(int col0, int &score, unsigned long long &key) const {
    int b = 0;
    unsigned long long kb = ~0ull;
#pragma unroll
    for (int c = 0; c < CPL; ++c)   // c ascending, strict >: the lowest column wins a tie
      if (s[c] > b) { b = s[c]; kb = ((unsigned long long)(uint32_t)(col0 + c) << 32) | (uint32_t)r[c]; }
    score = wave_max_i32(b);
    key = wave_min_u64(b == score && score > 0 ? kb : ~0ull);
    if (ret_s >= score && ret_s > 0) {   // a tie goes to the lower column: a retired one
      score = ret_s;
      key = ((unsigned long long)(uint32_t)ret_col << 32) | (uint32_t)ret_row;
    }
  }
};

// strip_publish, and one more publication counted in the pair's front word
__device__ __forceinline__ void band_publish(uint32_t *word, uint32_t *front, uint32_t value) {
  strip_publish(word, value);
  if (threadIdx.x == 0) __hip_atomic_fetch_add(front, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// strip_wait with a way out: false when `word` stayed below `need` and the pair's front word -- the count of publications by
// ANY of the pair's strips -- stood still for kBandWaitTicks (header)
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

// a wait ran dry: the pair is recorded (the first to give up stays) and the strips to my right fall through; the caller returns
__device__ __forceinline__ void band_give_up(uint32_t *give_up, uint32_t pair, uint32_t *word, uint32_t *front) {
  if (threadIdx.x == 0) atomicCAS(give_up, 0u, pair + 1u);
  band_publish(word, front, kAllRows);
}

// ---- the launch side
// the grid of a wide launch: one workgroup per (pair, strip), the pairs rounded up to the tickets' groups of 8
inline hipError_t band_strips_grid(uint32_t n_pairs, uint32_t strips_per_pair, dim3 &grid) {
  const uint64_t blocks = (uint64_t)((n_pairs + 7) / 8) * 8 * strips_per_pair;
  if (strips_per_pair == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  grid = dim3((unsigned)blocks);
  return hipSuccess;
}

// strip_cols = 64 x CPL: launch(std::integral_constant<int, CPL>{}) for 64 | 128 | 256 | 512, and what it returns
template <class F>
hipError_t launch_by_strip_cols(uint32_t strip_cols, F &&launch) {
  switch (strip_cols) {
    case 64: return launch(std::integral_constant<int, 1>{});
    case 128: return launch(std::integral_constant<int, 2>{});
    case 256: return launch(std::integral_constant<int, 4>{});
    case 512: return launch(std::integral_constant<int, 8>{});
  }
  return hipErrorInvalidValue;
}

}  // namespace sa
