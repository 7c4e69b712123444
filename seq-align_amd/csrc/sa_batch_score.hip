// sa_batch_score.hip -- score only over HOST batches: seqalign_nw_score_batch, seqalign_sw_score_batch (and the timing
// hook seqalign_score_time_ms).  No matrices, no traceback: per chunk the sequences go up, the score kernels
// (sa_score.hip) run, 4 or 12 bytes per pair come back.
//
// A chunk's pairs are put in classes by row width -- the columns per lane of the one-wave kernel (1 .. 16), or the strips
// kernel for rows over 1 024 columns -- and the descriptors are laid out class by class, so that each class is one launch
// that sizes its registers to its own widest row (a ragged batch does not run its short rows at 16 columns per lane).  The
// sequences stay in pair order; the results are put back in pair order on the host.
//
// Chunks are cut by device BYTES, not cells: the sequences, 64 bytes of descriptors, status and results per pair, and for
// the strips kernel the hand-off columns (8 bytes per row and strip) -- a 100 000 x 100 000 pair is 157 MB, not 120 GB.
#include "sa_ctx.hpp"

using namespace sa_host;

namespace {

constexpr int kRowClasses = SA_SCORE_ROW_CLASSES;   // sa_score.hip's instantiations (sa_score_row_class)
constexpr int kStripClass = kRowClasses;           // rows over SA_SCORE_ROW_MAX columns
constexpr uint64_t kPairBytes = 64;   // descriptors (32), results (12), status (8), slack
constexpr uint64_t kChunkMaxPairs = (uint64_t)1 << 24;

// hand-off columns of one pair: strips 0 .. last - 1, len_b + 1 rows each, in int2 units
uint64_t handoff_rows(uint32_t la, uint32_t lb) {
  return la > SA_SCORE_ROW_MAX ? (uint64_t)(sa_score_strips_per_pair(la) - 1) * ((uint64_t)lb + 1) : 0;
}

struct ScoreChunk {
  uint64_t first = 0, count = 0, seq_bytes = 0;
};

// plan_chunks' sibling: bytes of sequences + what each pair needs besides, no per-cell term
std::vector<ScoreChunk> plan_score_chunks(const seqalign_batch_t *b, size_t budget) {
  std::vector<ScoreChunk> out;
  ScoreChunk c;
  uint64_t used = 0;
  for (uint64_t p = 0; p < b->n_pairs; ++p) {
    const uint32_t la = b->len_a[p], lb = b->len_b[p];
    const uint64_t strips = la > SA_SCORE_ROW_MAX ? sa_score_strips_per_pair(la) : 0;
    const uint64_t need = (uint64_t)la + lb + kPairBytes + 8 * handoff_rows(la, lb) + 20 * strips;
    if (c.count && (used + need > budget || c.count == kChunkMaxPairs)) { out.push_back(c); c = ScoreChunk(); c.first = p; used = 0; }
    used += need;
    c.count++; c.seq_bytes += (uint64_t)la + lb;
  }
  if (c.count) out.push_back(c);
  return out;
}

}  // namespace

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

// One chunk laid out and uploaded; launch() enqueues its kernels on ctx->stream (repeatable: it re-zeroes what they count on)
struct ScoreChunkRun {
  seqalign_ctx *ctx = nullptr;
  const seqalign_dev_scoring *sc = nullptr;
  bool is_sw = false;
  uint64_t n = 0;
  std::vector<uint32_t> order;                 // descriptor slot -> pair of the chunk
  uint64_t cls_first[kRowClasses + 2] = {};    // class c: slots [cls_first[c], cls_first[c + 1])
  uint32_t cls_max_a[kRowClasses + 1] = {};
  uint32_t spp = 1;                            // strips per pair of the strips class
  uint64_t strip_words = 0;                    // its progress words
  uint64_t *d_off_a = nullptr, *d_off_b = nullptr, *d_hoff = nullptr;
  uint32_t *d_len_a = nullptr, *d_len_b = nullptr;
  uint32_t *d_res = nullptr;                   // [4] header (err_flag), then score[n], end_a[n], end_b[n]

  int prepare(const seqalign_batch_t *b, const ScoreChunk &c) {
    int rc;
    n = c.count;
    uint64_t hand_total = 0;
    order.resize(n);
    sort_by_row_class(n, [&](uint64_t k) { return b->len_a[c.first + k]; }, order.data(), cls_first, cls_max_a);
    const uint64_t n_strip = cls_first[kStripClass + 1] - cls_first[kStripClass];
    spp = n_strip ? sa_score_strips_per_pair(cls_max_a[kStripClass]) : 1;
    strip_words = ((n_strip + 7) / 8) * 8 * spp;

    // pinned descriptors, slot order: off_a, off_b, handoff_off (u64), len_a, len_b (u32); sequences in pair order
    const size_t desc_bytes = n * (3 * sizeof(uint64_t) + 2 * sizeof(uint32_t));
    if ((rc = ctx->h_desc.reserve(desc_bytes)) || (rc = ctx->h_arena.reserve(c.seq_bytes + 16))) return rc;
    uint64_t *h_off_a = ctx->h_desc.as<uint64_t>(), *h_off_b = h_off_a + n, *h_hoff = h_off_b + n;
    uint32_t *h_len_a = reinterpret_cast<uint32_t *>(h_hoff + n), *h_len_b = h_len_a + n;
    std::vector<uint64_t> seq_at(n);
    { uint64_t pos = 0;
      for (uint64_t k = 0; k < n; ++k) { seq_at[k] = pos; pos += (uint64_t)b->len_a[c.first + k] + b->len_b[c.first + k]; } }
    for (uint64_t s = 0; s < n; ++s) {
      const uint64_t k = order[s], p = c.first + k;
      const uint32_t la = b->len_a[p], lb = b->len_b[p];
      h_off_a[s] = seq_at[k]; h_off_b[s] = seq_at[k] + la;
      h_len_a[s] = la; h_len_b[s] = lb;
      h_hoff[s] = hand_total; hand_total += handoff_rows(la, lb);
    }
    uint8_t *h_seq = ctx->h_arena.as<uint8_t>();
    constexpr uint64_t kTask = 256;
    parallel_for((n + kTask - 1) / kTask, [&](uint64_t blk) {
      for (uint64_t k = blk * kTask, e = std::min(n, (blk + 1) * kTask); k < e; ++k) {
        const uint64_t p = c.first + k;
        memcpy(h_seq + seq_at[k], b->arena + b->off_a[p], b->len_a[p]);
        memcpy(h_seq + seq_at[k] + b->len_a[p], b->arena + b->off_b[p], b->len_b[p]);
      }
    });

    if ((rc = ctx->arena.reserve(c.seq_bytes + 16)) || (rc = ctx->off_a.reserve(desc_bytes)) || (rc = ctx->status.reserve(n * 8)) ||
        (rc = ctx->best_score.reserve(16 + 12 * n)))
      return rc;
    if (n_strip && ((rc = ctx->strip_progress.reserve(sa_strip_progress_bytes(strip_words))) ||
                    (rc = ctx->score_handoff.reserve(8 * hand_total + 16))))
      return rc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->off_a.p, h_off_a, desc_bytes, hipMemcpyHostToDevice, st));
    if (c.seq_bytes) HIP_TRY(hipMemcpyAsync(ctx->arena.p, h_seq, c.seq_bytes, hipMemcpyHostToDevice, st));
    d_off_a = ctx->off_a.as<uint64_t>(); d_off_b = d_off_a + n; d_hoff = d_off_b + n;
    d_len_a = reinterpret_cast<uint32_t *>(d_hoff + n); d_len_b = d_len_a + n;
    d_res = ctx->best_score.as<uint32_t>();
    return SEQALIGN_OK;
  }

  int launch() {
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(d_res, 0, 16, st));
    const SaFillParams f0 = score_fill_params(sc);
    for (int x = 0; x <= kRowClasses; ++x) {
      const uint64_t s0 = cls_first[x], m = cls_first[x + 1] - s0;
      if (!m) continue;
      SaScoreParams p;
      memset(&p, 0, sizeof(p));
      p.f = f0;
      p.f.arena = ctx->arena.as<uint8_t>();
      p.f.off_a = d_off_a + s0; p.f.off_b = d_off_b + s0; p.f.len_a = d_len_a + s0; p.f.len_b = d_len_b + s0;
      p.f.status = ctx->status.as<uint64_t>() + s0;
      p.f.n_pairs = (uint32_t)m;
      p.score = reinterpret_cast<int32_t *>(d_res + 4) + s0;
      p.end_a = d_res + 4 + n + s0; p.end_b = d_res + 4 + 2 * n + s0;
      p.err_flag = d_res;
      hipError_t e;
      if (x == kStripClass) {
        p.progress = ctx->strip_progress.as<uint32_t>();
        p.strip_best = p.progress + sa_strip_best_word(strip_words);
        p.handoff = ctx->score_handoff.as<int32_t>();
        p.handoff_off = d_hoff + s0;
        p.strips_per_pair = spp;
        HIP_TRY(hipMemsetAsync(p.progress, 0, 4 * (strip_words + 1), st));
        HIP_TRY(hipMemsetAsync(p.f.status, 0xff, 8 * m, st));
        e = sa_launch_score_strips(p, is_sw, st);
      } else {
        e = sa_launch_score_rows(p, cls_max_a[x], is_sw, st);
      }
      if (e != hipSuccess) return fail_hip(e, "score kernel launch");
    }
    return SEQALIGN_OK;
  }

  // results home, in pair order; the lowest failing pair of the chunk named
  int finish(uint64_t first, int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b, uint64_t *fail_pair = nullptr) {
    int rc;
    const size_t words = 4 + (is_sw ? 3 : 1) * n;
    if ((rc = ctx->h_misc.reserve(std::max<size_t>(4 * words, 8 * n)))) return rc;
    uint32_t *h = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h, d_res, 4 * words, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    if (h[0]) {
      std::vector<uint64_t> status(n);
      HIP_TRY(hipMemcpy(status.data(), ctx->status.p, 8 * n, hipMemcpyDeviceToHost));
      uint64_t worst = ~0ull;
      for (uint64_t s = 0; s < n; ++s)
        if (status[s] != ~0ull) worst = std::min<uint64_t>(worst, order[s]);
      if (fail_pair) *fail_pair = first + worst;
      return fail_unknown_pair(first + worst);
    }
    const int32_t *hs = reinterpret_cast<const int32_t *>(h + 4);
    const uint32_t *ha = h + 4 + n, *hb = h + 4 + 2 * n;
    constexpr uint64_t kTask = 16384;
    parallel_for((n + kTask - 1) / kTask, [&](uint64_t blk) {
      for (uint64_t s = blk * kTask, e = std::min(n, (blk + 1) * kTask); s < e; ++s) {
        const uint64_t p = first + order[s];
        out_score[p] = hs[s];
        if (is_sw) { out_end_a[p] = ha[s]; out_end_b[p] = hb[s]; }
      }
    });
    return SEQALIGN_OK;
  }
};

int check_score_batch(const seqalign_batch_t *b) {   // check_batch without the 2^31-cell cap
  if (!batch_readable(b)) return SEQALIGN_E_ARG;
  return SEQALIGN_OK;
}

}  // namespace

int sa_host::score_batch_impl(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, bool is_sw,
                              int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b, uint64_t *fail_pair) {
  int rc = check_score_batch(batch);
  if (rc) return rc;
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, is_sw ? 1 : 0, &sc))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  for (const ScoreChunk &c : plan_score_chunks(batch, ctx->chunk_budget)) {
    ScoreChunkRun run;
    run.ctx = ctx; run.sc = sc; run.is_sw = is_sw;
    if ((rc = run.prepare(batch, c)) || (rc = run.launch()) ||
        (rc = run.finish(c.first, out_score, out_end_a, out_end_b, fail_pair)))
      return rc;
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
  int rc = check_score_batch(batch);
  if (rc) return rc;
  if (batch->n_pairs == 0) return SEQALIGN_E_ARG;
  const std::vector<ScoreChunk> chunks = plan_score_chunks(batch, ctx->chunk_budget);
  if (chunks.size() != 1) { set_last_error("seqalign_score_time_ms: the batch does not fit one chunk"); return SEQALIGN_E_ARG; }
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, is_sw ? 1 : 0, &sc))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  ScoreChunkRun run;
  run.ctx = ctx; run.sc = sc; run.is_sw = is_sw != 0;
  if ((rc = run.prepare(batch, chunks[0]))) return rc;
  EventList events;
  for (int r = 0; r < 2 * repeats; ++r) HIP_TRY(events.add());
  for (int r = 0; r < repeats; ++r) {
    HIP_TRY(hipEventRecord(events.ev[2 * r], ctx->stream));
    if ((rc = run.launch())) return rc;
    HIP_TRY(hipEventRecord(events.ev[2 * r + 1], ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (int r = 0; r < repeats; ++r) HIP_TRY(hipEventElapsedTime(&ms_each[r], events.ev[2 * r], events.ev[2 * r + 1]));
  return SEQALIGN_OK;
}
