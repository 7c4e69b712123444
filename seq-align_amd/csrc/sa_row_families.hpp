// sa_row_families.hpp -- the families of row-sweep calls that keep nothing per cell, one traits struct each: what the batch
// driver (RowChunkRun, sa_batch_score.hip) and the cross driver (CrossCall, sa_batch_score_cross.hip) need to know of a family --
// the kernels' parameter block, ladder and launch functions, the result words per pair and the bytes the chunk and tile cuts
// count.  DESIGN.md 3.23.  Host code only.
#pragma once
#include "sa_chunks.hpp"

namespace sa_host {

struct ScoreTraits {   // sa_score.hip
  using Params = SaScoreParams;
  using CrossParams = SaCrossParams<Params>;   // the one-wave kernel's form over two sets (sa_batch_score_cross.hip)
  static constexpr int kRowClasses = SA_SCORE_ROW_CLASSES;   // its instantiations (sa_score_row_class)
  static constexpr uint32_t kRowMax = SA_SCORE_ROW_MAX;
  static constexpr uint64_t kPairBytes = 64;   // descriptors (32), results (12), status (8), slack
  static constexpr uint64_t kHandoffBytes = 8, kBestBytes = 16;
  static constexpr const char *kLaunch = "score kernel launch", *kLaunchCross = "score cross kernel launch";
  static constexpr int kMarkField = 0;         // no result word carries a mark
  static int fields(bool is_sw) { return is_sw ? 3 : 1; }   // result words per pair: score; SW: end_a, end_b
  static int row_class(uint32_t la) { return sa_score_row_class(la); }
  static uint32_t strips_per_pair(uint32_t la) { return sa_score_strips_per_pair(la); }
  static void set_results(Params &p, uint32_t *res, uint64_t n) { p.end_a = res + n; p.end_b = res + 2 * n; }
  static void set_strip_best(Params &p, uint32_t *best) { p.strip_best = best; }
  static hipError_t launch_rows(const Params &p, uint32_t max_a, bool is_sw, hipStream_t st) { return sa_launch_score_rows(p, max_a, is_sw, st); }
  static hipError_t launch_strips(const Params &p, bool is_sw, hipStream_t st) { return sa_launch_score_strips(p, is_sw, st); }
  static hipError_t launch_cross(const CrossParams &p, uint32_t max_a, bool is_sw, hipStream_t st) { return sa_launch_score_cross(p, max_a, is_sw, st); }
};

struct SpanTraits {   // sa_span.hip: the SW form only
  using Params = SaSpanParams;
  using CrossParams = SaCrossParams<Params>;
  static constexpr int kRowClasses = SA_SPAN_ROW_CLASSES;   // its instantiations (sa_span_row_class)
  static constexpr uint32_t kRowMax = SA_SPAN_ROW_MAX;
  static constexpr uint64_t kPairBytes = 72;   // descriptors (32), results (20), status (8), slack
  static constexpr uint64_t kHandoffBytes = SA_SPAN_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static constexpr const char *kLaunch = "span kernel launch", *kLaunchCross = "span cross kernel launch";
  static constexpr int kMarkField = 0;
  static int fields(bool) { return 5; }   // score, pos_a, pos_b, len_a, len_b
  static int row_class(uint32_t la) { return sa_span_row_class(la); }
  static uint32_t strips_per_pair(uint32_t la) { return sa_span_strips_per_pair(la); }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
  }
  static void set_strip_best(Params &p, uint32_t *best) { p.strip_best = best; }
  static hipError_t launch_rows(const Params &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_span_rows(p, max_a, st); }
  static hipError_t launch_strips(const Params &p, bool, hipStream_t st) { return sa_launch_span_strips(p, st); }
  static hipError_t launch_cross(const CrossParams &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_span_cross(p, max_a, st); }
};

struct StatsTraits {   // sa_nw_stats.hip: the NW form only; classes, strips and hand-off of the span kernels, no best cell
  using Params = SaStatsParams;
  using CrossParams = SaCrossParams<Params>;
  static constexpr int kRowClasses = SA_SPAN_ROW_CLASSES;
  static constexpr uint32_t kRowMax = SA_SPAN_ROW_MAX;
  static constexpr uint64_t kPairBytes = 64;   // descriptors (32), results (12), status (8), slack
  static constexpr uint64_t kHandoffBytes = SA_SPAN_HANDOFF_BYTES, kBestBytes = 0;
  static constexpr const char *kLaunch = "stats kernel launch", *kLaunchCross = "stats cross kernel launch";
  static constexpr int kMarkField = 2;         // SA_STATS_NO_WALK in the mismatch word: SEQALIGN_E_TRACEBACK
  static int fields(bool) { return 3; }   // score, matches, mismatches
  static int row_class(uint32_t la) { return sa_span_row_class(la); }
  static uint32_t strips_per_pair(uint32_t la) { return sa_span_strips_per_pair(la); }
  static void set_results(Params &p, uint32_t *res, uint64_t n) { p.matches = res + n; p.mismatches = res + 2 * n; }
  static void set_strip_best(Params &, uint32_t *) {}
  static hipError_t launch_rows(const Params &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_stats_rows(p, max_a, st); }
  static hipError_t launch_strips(const Params &p, bool, hipStream_t st) { return sa_launch_stats_strips(p, st); }
  static hipError_t launch_cross(const CrossParams &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_stats_cross(p, max_a, st); }
};

struct SwStatsTraits {   // sa_sw_stats.hip: the span kernels' classes, strips, hand-off and best-cell bytes; seven result words
  using Params = SaSwStatsParams;
  using CrossParams = SaCrossParams<Params>;
  static constexpr int kRowClasses = SA_SPAN_ROW_CLASSES;
  static constexpr uint32_t kRowMax = SA_SPAN_ROW_MAX;
  static constexpr uint64_t kPairBytes = 80;   // descriptors (32), results (28), status (8), slack
  static constexpr uint64_t kHandoffBytes = SA_SPAN_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static constexpr const char *kLaunch = "sw stats kernel launch", *kLaunchCross = "sw stats cross kernel launch";
  static constexpr int kMarkField = 0;
  static int fields(bool) { return 7; }   // score, pos_a, pos_b, len_a, len_b, matches, mismatches
  static int row_class(uint32_t la) { return sa_span_row_class(la); }
  static uint32_t strips_per_pair(uint32_t la) { return sa_span_strips_per_pair(la); }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
    p.matches = res + 5 * n; p.mismatches = res + 6 * n;
  }
  static void set_strip_best(Params &p, uint32_t *best) { p.strip_best = best; }
  static hipError_t launch_rows(const Params &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_sw_stats_rows(p, max_a, st); }
  static hipError_t launch_strips(const Params &p, bool, hipStream_t st) { return sa_launch_sw_stats_strips(p, st); }
  static hipError_t launch_cross(const CrossParams &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_sw_stats_cross(p, max_a, st); }
};

struct SwCountsTraits {   // sa_sw_counts.hip: the span kernels' classes, strips, hand-off, best-cell bytes and five result words
  using Params = SaSwCountsParams;
  static constexpr int kRowClasses = SA_SPAN_ROW_CLASSES;
  static constexpr uint32_t kRowMax = SA_SPAN_ROW_MAX;
  static constexpr uint64_t kPairBytes = 72;   // descriptors (32), results (20), status (8), slack
  static constexpr uint64_t kHandoffBytes = SA_SPAN_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static constexpr const char *kLaunch = "sw counts kernel launch";
  static constexpr int kMarkField = 0;
  static int fields(bool) { return 5; }   // score, end_a, end_b, matches, mismatches
  static int row_class(uint32_t la) { return sa_span_row_class(la); }
  static uint32_t strips_per_pair(uint32_t la) { return sa_span_strips_per_pair(la); }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {   // the span block's arrays by their new names (sa_kernels.h)
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
  }
  static void set_strip_best(Params &p, uint32_t *best) { p.strip_best = best; }
  static hipError_t launch_rows(const Params &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_sw_counts_rows(p, max_a, st); }
  static hipError_t launch_strips(const Params &p, bool, hipStream_t st) { return sa_launch_sw_counts_strips(p, st); }
  // no cross form: nothing for the cross driver to instantiate
};

struct SwGapsTraits {   // sa_sw_gaps.hip: SwCountsTraits with the gap-run kernels -- the span kernels' classes, strips and bytes
  using Params = SaSwGapsParams;
  static constexpr int kRowClasses = SA_SPAN_ROW_CLASSES;
  static constexpr uint32_t kRowMax = SA_SPAN_ROW_MAX;
  static constexpr uint64_t kPairBytes = 72;   // descriptors (32), results (20), status (8), slack
  static constexpr uint64_t kHandoffBytes = SA_SPAN_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static constexpr const char *kLaunch = "sw gaps kernel launch";
  static constexpr int kMarkField = 0;
  static int fields(bool) { return 5; }   // score, end_a, end_b, gap_runs_a, gap_runs_b
  static int row_class(uint32_t la) { return sa_span_row_class(la); }
  static uint32_t strips_per_pair(uint32_t la) { return sa_span_strips_per_pair(la); }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {   // the span block's arrays by their new names (sa_kernels.h)
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
  }
  static void set_strip_best(Params &p, uint32_t *best) { p.strip_best = best; }
  static hipError_t launch_rows(const Params &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_sw_gaps_rows(p, max_a, st); }
  static hipError_t launch_strips(const Params &p, bool, hipStream_t st) { return sa_launch_sw_gaps_strips(p, st); }
  // no cross form: nothing for the cross driver to instantiate
};

struct NwGapsTraits : StatsTraits {   // sa_nw_gaps.hip: StatsTraits with the gap-run kernels -- its classes, strips, bytes and cross
  // params; the result words are score, gap_runs_a, gap_runs_b, and kMarkField = 2 is SA_STATS_NO_WALK in the gap_runs_b word
  static constexpr const char *kLaunch = "nw gaps kernel launch", *kLaunchCross = "nw gaps cross kernel launch";
  static hipError_t launch_rows(const Params &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_nw_gaps_rows(p, max_a, st); }
  static hipError_t launch_strips(const Params &p, bool, hipStream_t st) { return sa_launch_nw_gaps_strips(p, st); }
  static hipError_t launch_cross(const CrossParams &p, uint32_t max_a, bool, hipStream_t st) { return sa_launch_nw_gaps_cross(p, max_a, st); }
};

// A family's batch call behind its entry checks: every chunk prepared, launched, brought home (sa_batch_score.hip, which
// instantiates it for the seven families).  out: the arrays behind the score, T::fields(is_sw) - 1 of them; fail_pair
// (optional): the failing pair it names, for SEQALIGN_E_TRACEBACK too.
template <class T>
int row_batch_call(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, bool is_sw, int32_t *out_score,
                   uint32_t *const *out, uint64_t *fail_pair = nullptr);

// One context's cross call of a family (its own CallScope; sa_batch_score_cross.hip, which instantiates it for the five).  The
// caller has checked the sets (score_cross_check).
struct CrossArgs {
  seqalign_ctx_t *ctx;
  const seqalign_seqset_t *queries, *targets;
  const scoring_t *scoring;
  bool is_sw;                 // the score family has both forms; the others their own
  int32_t *out_score;         // [n_queries * n_targets], and the matrices behind it, T::fields(is_sw) - 1 of them
  uint32_t *const *out_w;
  uint64_t q_base;            // what the error message adds to a query index (the *_multi calls' ranges)
};
template <class T>
int cross_call(const CrossArgs &a);

}  // namespace sa_host
