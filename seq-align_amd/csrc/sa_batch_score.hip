// sa_batch_score.hip -- score only over HOST batches: seqalign_nw_score_batch, seqalign_sw_score_batch (and the timing
// hook seqalign_score_time_ms), SW hit spans: seqalign_sw_span_batch (and seqalign_sw_span_time_ms), and NW alignment statistics:
// seqalign_nw_stats_batch (and seqalign_nw_stats_time_ms), and SW alignment statistics: seqalign_sw_stats_batch (and
// seqalign_sw_stats_time_ms), and SW identity counts at any length: seqalign_sw_counts_batch (and seqalign_sw_counts_time_ms), and SW
// gap-run counts at any length: seqalign_sw_gaps_batch (and seqalign_sw_gaps_time_ms), and NW gap-run counts: seqalign_nw_gaps_batch (and
// seqalign_nw_gaps_time_ms).  No matrices, no traceback: per chunk the sequences go up, the score kernels (sa_score.hip), the span
// kernels (sa_span.hip) or the stats kernels (sa_nw_stats.hip, sa_sw_stats.hip, sa_sw_counts.hip, sa_sw_gaps.hip, sa_nw_gaps.hip) run, and 4 or 12 bytes per pair come back, 20 for
// a span (score, pos_a, pos_b, len_a, len_b), 12 for NW statistics (score, matches, mismatches), 28 for SW statistics (the span's
// five, matches, mismatches), 20 for SW counts (score, end_a, end_b, matches, mismatches), 20 for SW gap runs (score, end_a, end_b, gap_runs_a,
// gap_runs_b), 12 for NW gap runs (score, gap_runs_a, gap_runs_b), plus the error word.
//
// A chunk's pairs are put in classes by row width -- the columns per lane of the one-wave kernel (score: 1 .. 16, span: 1 .. 6
// and 8), or the strips kernel for rows over 1 024 (span: 512) columns -- and the descriptors are laid out class by class, so
// that each class is one launch that sizes its registers to its own widest row (a ragged batch does not run its short rows at
// 16 columns per lane).  The sequences stay in pair order; the results are put back in pair order on the host.
//
// Chunks are cut by device BYTES, not cells (sa_chunks.hpp): the sequences, 64 (span: 72) bytes of descriptors, status and
// results per pair, and for the strips kernel the hand-off columns (8 bytes per row and strip; span: 32) and 20 (span: 36)
// bytes per strip of progress and best cell -- a 100 000 x 100 000 score pair is 157 MB, not 120 GB.  Statistics: 64 bytes per
// pair, the span's 32 per row and strip, 4 per strip (no best cell).  SW statistics: the span's bytes plus 8 of results per pair
// (80), its 32 per row and strip and its 36 per strip.  SW counts and SW gap runs: the span's bytes exactly.
//
// The six families are one driver (RowChunkRun) over a traits struct each (sa_row_families.hpp, shared with the cross driver):
// what differs is the kernels' parameter block, ladder and launch functions and the bytes named above.
#include "sa_row_families.hpp"

using namespace sa_host;

SaFillParams sa_host::score_fill_params(const seqalign_dev_scoring *s) {
  SaFillParams p;
  memset(&p, 0, sizeof(p));
  p.code = s->d_code; p.table = s->d_table; p.K = s->flat.n_classes;
  p.gap_open = s->flat.gap_open; p.open1 = s->flat.open1; p.ext = s->flat.ext; p.floor = s->flat.floor;
  p.gen_eq = s->flat.gen_eq; p.gen_ne = s->flat.gen_ne; p.flags = s->flat.flags;
  p.table_abs_max = s->table_abs_max;
  return p;
}

namespace {

// hand-off columns of one pair: strips 0 .. last - 1, len_b + 1 rows each, in rows
template <class T>
uint64_t handoff_rows(uint32_t la, uint32_t lb) {
  return la > T::kRowMax ? (uint64_t)(T::strips_per_pair(la) - 1) * ((uint64_t)lb + 1) : 0;
}

// plan_chunks' sibling: bytes of sequences + what each pair needs besides, no per-cell term.  A pair over the budget alone
// is a chunk of its own
template <class T>
std::vector<ByteChunk> plan_row_chunks(const seqalign_batch_t *b, size_t budget) {
  std::vector<ByteChunk> out;
  (void)cut_chunks(b, budget, [&](uint64_t p) {
    const uint32_t la = b->len_a[p], lb = b->len_b[p];
    const uint64_t strips = la > T::kRowMax ? T::strips_per_pair(la) : 0;
    return PairNeed{(uint64_t)la + lb + T::kPairBytes + T::kHandoffBytes * handoff_rows<T>(la, lb) + (4 + T::kBestBytes) * strips};
  }, out);
  return out;
}

// One chunk laid out and uploaded; launch() enqueues its kernels on ctx->stream (repeatable: it re-zeroes what they count on)
template <class T>
struct RowChunkRun {
  static constexpr int kStripClass = T::kRowClasses;   // rows over T::kRowMax columns
  const seqalign_dev_scoring *sc = nullptr;
  bool is_sw = false;
  ChunkStage<T::kRowClasses> stage;   // classes by len_a; the caller's array: handoff_off
  uint64_t n = 0;
  uint32_t spp = 1;                   // strips per pair of the strips class
  uint64_t strip_words = 0;           // its progress words
  uint32_t *d_res = nullptr;          // [4] header (err_flag), then T::fields arrays of n words: score first

  RowChunkRun(seqalign_ctx *ctx, const seqalign_dev_scoring *scoring, bool sw) : sc(scoring), is_sw(sw) { stage.ctx = ctx; }

  int prepare(const seqalign_batch_t *b, const ByteChunk &c) {
    int rc;
    seqalign_ctx *ctx = stage.ctx;
    n = c.count;
    uint64_t hand_total = 0;
    rc = stage.lay_out(b, c, T::row_class, [&](uint64_t p) { return b->len_a[p]; }, 1, 0, [&](uint64_t s, uint64_t p) {
      stage.h_u64(0)[s] = hand_total; hand_total += handoff_rows<T>(b->len_a[p], b->len_b[p]);
    });
    if (rc) return rc;
    const uint64_t n_strip = stage.class_size(kStripClass);
    spp = n_strip ? T::strips_per_pair(stage.cls_max[kStripClass]) : 1;
    strip_words = ((n_strip + 7) / 8) * 8 * spp;
    if ((rc = ctx->best_score.reserve(16 + 4 * T::fields(true) * n))) return rc;
    if (n_strip && ((rc = ctx->strip_progress.reserve(4 * sa_strip_best_word(strip_words) + T::kBestBytes * strip_words)) ||
                    (rc = ctx->score_handoff.reserve(T::kHandoffBytes * hand_total + 16))))
      return rc;
    d_res = ctx->best_score.as<uint32_t>();
    return stage.upload();
  }

  int launch() {
    seqalign_ctx *ctx = stage.ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(d_res, 0, 16, st));
    const SaFillParams f0 = score_fill_params(sc);
    for (int x = 0; x <= T::kRowClasses; ++x) {
      const uint64_t s0 = stage.cls_first[x], m = stage.class_size(x);
      if (!m) continue;
      typename T::Params p;
      memset(&p, 0, sizeof(p));
      p.f = f0;
      stage.set_slots(p.f, s0, m);
      p.score = reinterpret_cast<int32_t *>(d_res + 4) + s0;
      T::set_results(p, d_res + 4 + s0, n);
      p.err_flag = d_res;
      hipError_t e;
      if (x == kStripClass) {
        p.progress = ctx->strip_progress.as<uint32_t>();
        T::set_strip_best(p, p.progress + sa_strip_best_word(strip_words));
        p.handoff = ctx->score_handoff.as<int32_t>();
        p.handoff_off = stage.d_u64(0) + s0;
        p.strips_per_pair = spp;
        HIP_TRY(hipMemsetAsync(p.progress, 0, 4 * (strip_words + 1), st));
        HIP_TRY(hipMemsetAsync(p.f.status, 0xff, 8 * m, st));
        e = T::launch_strips(p, is_sw, st);
      } else {
        e = T::launch_rows(p, stage.cls_max[x], is_sw, st);
      }
      if (e != hipSuccess) return fail_hip(e, T::kLaunch);
    }
    return SEQALIGN_OK;
  }

  // results home, in pair order (out: the arrays behind the score); the lowest failing pair of the chunk named
  int finish(int32_t *out_score, uint32_t *const *out, uint64_t *fail_pair) {
    int rc;
    seqalign_ctx *ctx = stage.ctx;
    const int fields = T::fields(is_sw);
    const size_t words = 4 + fields * n;
    if ((rc = ctx->h_misc.reserve(4 * words))) return rc;
    uint32_t *h = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h, d_res, 4 * words, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    uint64_t unknown = ~0ull, no_walk = ~0ull;   // the chunk's lowest failing pairs, as batch indices
    if (h[0] && (rc = stage.fail_from_status(&unknown)) != SEQALIGN_E_UNKNOWN_PAIR) return rc;
    if constexpr (T::kMarkField > 0) {   // stats: SA_STATS_NO_WALK in the mismatch word
      const uint32_t *w = h + 4 + (uint64_t)T::kMarkField * n;
      for (uint64_t s = 0; s < n; ++s)
        if (w[s] & SA_STATS_NO_WALK) no_walk = std::min<uint64_t>(no_walk, stage.first + stage.order[s]);
    }
    if (no_walk < unknown) {   // the lowest failing pair's code is the call's, as seqalign_nw_batch's; on one pair the fill's first
      if (fail_pair) *fail_pair = no_walk;
      set_last_error("pair " + std::to_string(no_walk) + ": traceback failed");
      return SEQALIGN_E_TRACEBACK;
    }
    if (h[0]) {
      if (fail_pair) *fail_pair = unknown;
      return SEQALIGN_E_UNKNOWN_PAIR;
    }
    stage.scatter(h + 4, fields, out_score, out);
    return SEQALIGN_OK;
  }
};

}  // namespace

// seqalign_*_score_batch / seqalign_sw_span_batch / seqalign_*_stats_batch behind their entry checks (sa_row_families.hpp)
template <class T>
int sa_host::row_batch_call(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, bool is_sw,
                            int32_t *out_score, uint32_t *const *out, uint64_t *fail_pair) {
  if (!batch_readable(batch)) return SEQALIGN_E_ARG;   // check_batch without the 2^31-cell cap
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  int rc;
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, is_sw ? 1 : 0, &sc))) return rc;
  if ((rc = admit_batch(sc, batch, SA_FRAMES_ROWS))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  for (const ByteChunk &c : plan_row_chunks<T>(batch, ctx->chunk_budget)) {
    RowChunkRun<T> run(ctx, sc, is_sw);
    if ((rc = run.prepare(batch, c)) || (rc = run.launch()) || (rc = run.finish(out_score, out, fail_pair))) return rc;
  }
  return SEQALIGN_OK;
}
template int sa_host::row_batch_call<ScoreTraits>(seqalign_ctx_t *, const seqalign_batch_t *, const scoring_t *, bool, int32_t *, uint32_t *const *, uint64_t *);
template int sa_host::row_batch_call<SpanTraits>(seqalign_ctx_t *, const seqalign_batch_t *, const scoring_t *, bool, int32_t *, uint32_t *const *, uint64_t *);
template int sa_host::row_batch_call<StatsTraits>(seqalign_ctx_t *, const seqalign_batch_t *, const scoring_t *, bool, int32_t *, uint32_t *const *, uint64_t *);
template int sa_host::row_batch_call<SwStatsTraits>(seqalign_ctx_t *, const seqalign_batch_t *, const scoring_t *, bool, int32_t *, uint32_t *const *, uint64_t *);
template int sa_host::row_batch_call<SwCountsTraits>(seqalign_ctx_t *, const seqalign_batch_t *, const scoring_t *, bool, int32_t *, uint32_t *const *, uint64_t *);
template int sa_host::row_batch_call<SwGapsTraits>(seqalign_ctx_t *, const seqalign_batch_t *, const scoring_t *, bool, int32_t *, uint32_t *const *, uint64_t *);
template int sa_host::row_batch_call<NwGapsTraits>(seqalign_ctx_t *, const seqalign_batch_t *, const scoring_t *, bool, int32_t *, uint32_t *const *, uint64_t *);

namespace {

// the launches of a batch that is one chunk, `repeats` times between HIP events; `name`: the hook's, for its message
template <class T>
int row_time_call(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, bool is_sw, int repeats, float *ms_each,
                  const char *name) {
  if (!batch_readable(batch) || batch->n_pairs == 0) return SEQALIGN_E_ARG;
  const std::vector<ByteChunk> chunks = plan_row_chunks<T>(batch, ctx->chunk_budget);
  if (chunks.size() != 1) { set_last_error(std::string(name) + ": the batch does not fit one chunk"); return SEQALIGN_E_ARG; }
  HIP_TRY(hipSetDevice(ctx->device));
  int rc;
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, is_sw ? 1 : 0, &sc))) return rc;
  if ((rc = admit_batch(sc, batch, SA_FRAMES_ROWS))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  RowChunkRun<T> run(ctx, sc, is_sw);
  if ((rc = run.prepare(batch, chunks[0]))) return rc;
  return time_launches(ctx->stream, repeats, ms_each, [&] { return run.launch(); });
}

}  // namespace

int sa_host::score_batch_impl(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, bool is_sw,
                              int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b, uint64_t *fail_pair) {
  uint32_t *const out[2] = {out_end_a, out_end_b};
  return row_batch_call<ScoreTraits>(ctx, batch, scoring, is_sw, out_score, out, fail_pair);
}

int sa_host::span_batch_impl(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int32_t *out_score,
                             uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b,
                             uint64_t *fail_pair) {
  uint32_t *const out[4] = {out_pos_a, out_pos_b, out_len_a, out_len_b};
  return row_batch_call<SpanTraits>(ctx, batch, scoring, true, out_score, out, fail_pair);
}

// seqalign_sw_stats_*'s length limit: a coordinate and a counter are 16 bits each in the kernels' payload words
int sa_host::sw_stats_check_batch(const seqalign_batch_t *batch) {
  for (uint64_t p = 0; p < batch->n_pairs; ++p)
    if (batch->len_a[p] > SEQALIGN_SW_STATS_MAX_LEN || batch->len_b[p] > SEQALIGN_SW_STATS_MAX_LEN) {
      const bool in_a = batch->len_a[p] > SEQALIGN_SW_STATS_MAX_LEN;
      set_last_error("pair " + std::to_string(p) + ": " + (in_a ? "seq_a" : "seq_b") + " has " +
                     std::to_string(in_a ? batch->len_a[p] : batch->len_b[p]) + " letters, SW statistics take at most " +
                     std::to_string(SEQALIGN_SW_STATS_MAX_LEN));
      return SEQALIGN_E_TOO_LARGE;
    }
  return SEQALIGN_OK;
}

extern "C" int seqalign_nw_score_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       int32_t *out_score) {
  if (!ctx || !scoring || !out_score) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return score_batch_impl(ctx, batch, scoring, false, out_score, nullptr, nullptr);
}

extern "C" int seqalign_sw_score_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b) {
  if (!ctx || !scoring || !out_score || !out_end_a || !out_end_b) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return score_batch_impl(ctx, batch, scoring, true, out_score, out_end_a, out_end_b);
}

extern "C" int seqalign_score_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int is_sw,
                                      int repeats, float *ms_each) {
  if (!ctx || !scoring || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return row_time_call<ScoreTraits>(ctx, batch, scoring, is_sw != 0, repeats, ms_each, "seqalign_score_time_ms");
}

extern "C" int seqalign_sw_span_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                      int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a,
                                      uint32_t *out_len_b) {
  if (!ctx || !scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return span_batch_impl(ctx, batch, scoring, out_score, out_pos_a, out_pos_b, out_len_a, out_len_b);
}

extern "C" int seqalign_sw_span_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                                        float *ms_each) {
  if (!ctx || !scoring || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return row_time_call<SpanTraits>(ctx, batch, scoring, true, repeats, ms_each, "seqalign_sw_span_time_ms");
}

extern "C" int seqalign_nw_stats_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches) {
  if (!ctx || !scoring || !out_score || !out_matches || !out_mismatches || !batch_readable(batch)) return SEQALIGN_E_ARG;
  CallScope scope(ctx);   // (every argument checked before the context is touched)
  uint32_t *const out[2] = {out_matches, out_mismatches};
  return row_batch_call<StatsTraits>(ctx, batch, scoring, false, out_score, out);
}

extern "C" int seqalign_nw_stats_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                                         float *ms_each) {
  if (!ctx || !scoring || repeats <= 0 || !ms_each || !batch_readable(batch) || batch->n_pairs == 0) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return row_time_call<StatsTraits>(ctx, batch, scoring, false, repeats, ms_each, "seqalign_nw_stats_time_ms");
}

// NW gap-run counts: seqalign_nw_stats_batch's checks in its order
extern "C" int seqalign_nw_gaps_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                      int32_t *out_score, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b) {
  if (!ctx || !scoring || !out_score || !out_gap_runs_a || !out_gap_runs_b || !batch_readable(batch)) return SEQALIGN_E_ARG;
  CallScope scope(ctx);   // (every argument checked before the context is touched)
  uint32_t *const out[2] = {out_gap_runs_a, out_gap_runs_b};
  return row_batch_call<NwGapsTraits>(ctx, batch, scoring, false, out_score, out);
}

extern "C" int seqalign_nw_gaps_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                                        float *ms_each) {
  if (!ctx || !scoring || repeats <= 0 || !ms_each || !batch_readable(batch) || batch->n_pairs == 0) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return row_time_call<NwGapsTraits>(ctx, batch, scoring, false, repeats, ms_each, "seqalign_nw_gaps_time_ms");
}

extern "C" int seqalign_sw_stats_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a,
                                       uint32_t *out_len_b, uint32_t *out_matches, uint32_t *out_mismatches) {
  if (!scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b || !out_matches || !out_mismatches ||
      !batch_readable(batch))
    return SEQALIGN_E_ARG;
  int rc = sw_stats_check_batch(batch);   // (before the context is looked at: the limit is the arguments' own)
  if (rc) return rc;
  if (!ctx) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  uint32_t *const out[6] = {out_pos_a, out_pos_b, out_len_a, out_len_b, out_matches, out_mismatches};
  return row_batch_call<SwStatsTraits>(ctx, batch, scoring, true, out_score, out);
}

extern "C" int seqalign_sw_stats_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                                         float *ms_each) {
  if (!scoring || repeats <= 0 || !ms_each || !batch_readable(batch) || batch->n_pairs == 0) return SEQALIGN_E_ARG;
  int rc = sw_stats_check_batch(batch);
  if (rc) return rc;
  if (!ctx) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return row_time_call<SwStatsTraits>(ctx, batch, scoring, true, repeats, ms_each, "seqalign_sw_stats_time_ms");
}

// SW identity counts at any length: seqalign_sw_span_batch's checks in its order, no length limit
extern "C" int seqalign_sw_counts_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b, uint32_t *out_matches,
                                        uint32_t *out_mismatches) {
  if (!ctx || !scoring || !out_score || !out_end_a || !out_end_b || !out_matches || !out_mismatches || !batch_readable(batch))
    return SEQALIGN_E_ARG;
  CallScope scope(ctx);   // (every argument checked before the context is touched)
  uint32_t *const out[4] = {out_end_a, out_end_b, out_matches, out_mismatches};
  return row_batch_call<SwCountsTraits>(ctx, batch, scoring, true, out_score, out);
}

extern "C" int seqalign_sw_counts_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                                          float *ms_each) {
  if (!ctx || !scoring || repeats <= 0 || !ms_each || !batch_readable(batch) || batch->n_pairs == 0) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return row_time_call<SwCountsTraits>(ctx, batch, scoring, true, repeats, ms_each, "seqalign_sw_counts_time_ms");
}

// SW gap-run counts at any length: seqalign_sw_counts_batch's checks in its order (the span call's), no length limit
extern "C" int seqalign_sw_gaps_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                      int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b, uint32_t *out_gap_runs_a,
                                      uint32_t *out_gap_runs_b) {
  if (!ctx || !scoring || !out_score || !out_end_a || !out_end_b || !out_gap_runs_a || !out_gap_runs_b || !batch_readable(batch))
    return SEQALIGN_E_ARG;
  CallScope scope(ctx);   // (every argument checked before the context is touched)
  uint32_t *const out[4] = {out_end_a, out_end_b, out_gap_runs_a, out_gap_runs_b};
  return row_batch_call<SwGapsTraits>(ctx, batch, scoring, true, out_score, out);
}

extern "C" int seqalign_sw_gaps_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                                        float *ms_each) {
  if (!ctx || !scoring || repeats <= 0 || !ms_each || !batch_readable(batch) || batch->n_pairs == 0) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return row_time_call<SwGapsTraits>(ctx, batch, scoring, true, repeats, ms_each, "seqalign_sw_gaps_time_ms");
}
