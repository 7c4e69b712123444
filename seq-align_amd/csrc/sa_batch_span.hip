// sa_batch_span.hip -- SW hit spans over HOST batches: seqalign_sw_span_batch (and the timing hook
// seqalign_sw_span_time_ms).  sa_batch_score.hip's plan with the span kernels (sa_span.hip): per chunk the sequences go up,
// the kernels run, 20 bytes per pair come back (score, pos_a, pos_b, len_a, len_b) plus the error word.
//
// A chunk's pairs are put in classes by row width -- the columns per lane of the one-wave kernel (1 .. 6, 8), or the strips
// kernel for rows over 512 columns -- and the descriptors are laid out class by class: one launch per class.  The sequences
// stay in pair order; the results are put back in pair order on the host.
//
// Chunks are cut by device BYTES: the sequences, 72 bytes of descriptors, status and results per pair, and for the strips
// kernel the hand-off columns (32 bytes per row and strip) and 36 bytes per strip of progress and best cell.
#include "sa_ctx.hpp"

using namespace sa_host;

namespace {

constexpr int kRowClasses = SA_SPAN_ROW_CLASSES;   // sa_span.hip's instantiations (sa_span_row_class)
constexpr int kStripClass = kRowClasses;          // rows over SA_SPAN_ROW_MAX columns
constexpr uint64_t kPairBytes = 72;   // descriptors (32), results (20), status (8), slack
constexpr uint64_t kChunkMaxPairs = (uint64_t)1 << 24;

// hand-off columns of one pair: strips 0 .. last - 1, len_b + 1 rows each, in rows
uint64_t handoff_rows(uint32_t la, uint32_t lb) {
  return la > SA_SPAN_ROW_MAX ? (uint64_t)(sa_span_strips_per_pair(la) - 1) * ((uint64_t)lb + 1) : 0;
}

struct SpanChunk {
  uint64_t first = 0, count = 0, seq_bytes = 0;
};

// plan_chunks' sibling: bytes of sequences + what each pair needs besides, no per-cell term
std::vector<SpanChunk> plan_span_chunks(const seqalign_batch_t *b, size_t budget) {
  std::vector<SpanChunk> out;
  SpanChunk c;
  uint64_t used = 0;
  for (uint64_t p = 0; p < b->n_pairs; ++p) {
    const uint32_t la = b->len_a[p], lb = b->len_b[p];
    const uint64_t strips = la > SA_SPAN_ROW_MAX ? sa_span_strips_per_pair(la) : 0;
    const uint64_t need = (uint64_t)la + lb + kPairBytes + SA_SPAN_HANDOFF_BYTES * handoff_rows(la, lb) + (4 + SA_SPAN_BEST_BYTES) * strips;
    if (c.count && (used + need > budget || c.count == kChunkMaxPairs)) { out.push_back(c); c = SpanChunk(); c.first = p; used = 0; }
    used += need;
    c.count++; c.seq_bytes += (uint64_t)la + lb;
  }
  if (c.count) out.push_back(c);
  return out;
}

// One chunk laid out and uploaded; launch() enqueues its kernels on ctx->stream (repeatable: it re-zeroes what they count on)
struct SpanChunkRun {
  seqalign_ctx *ctx = nullptr;
  const seqalign_dev_scoring *sc = nullptr;
  uint64_t n = 0;
  std::vector<uint32_t> order;                 // descriptor slot -> pair of the chunk
  uint64_t cls_first[kRowClasses + 2] = {};    // class c: slots [cls_first[c], cls_first[c + 1])
  uint32_t cls_max_a[kRowClasses + 1] = {};
  uint32_t spp = 1;                            // strips per pair of the strips class
  uint64_t strip_words = 0;                    // its progress words
  uint64_t *d_off_a = nullptr, *d_off_b = nullptr, *d_hoff = nullptr;
  uint32_t *d_len_a = nullptr, *d_len_b = nullptr;
  uint32_t *d_res = nullptr;                   // [4] header (err_flag), then score, pos_a, pos_b, len_a, len_b [n] each

  int prepare(const seqalign_batch_t *b, const SpanChunk &c) {
    int rc;
    n = c.count;
    uint64_t hand_total = 0;
    order.resize(n);
    sort_by_class<kRowClasses>(n, sa_span_row_class, [&](uint64_t k) { return b->len_a[c.first + k]; }, order.data(), cls_first, cls_max_a);
    const uint64_t n_strip = cls_first[kStripClass + 1] - cls_first[kStripClass];
    spp = n_strip ? sa_span_strips_per_pair(cls_max_a[kStripClass]) : 1;
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
        (rc = ctx->best_score.reserve(16 + 20 * n)))
      return rc;
    if (n_strip && ((rc = ctx->strip_progress.reserve(sa_span_progress_bytes(strip_words))) ||
                    (rc = ctx->score_handoff.reserve(SA_SPAN_HANDOFF_BYTES * hand_total + 16))))
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
      SaSpanParams p;
      memset(&p, 0, sizeof(p));
      p.f = f0;
      p.f.arena = ctx->arena.as<uint8_t>();
      p.f.off_a = d_off_a + s0; p.f.off_b = d_off_b + s0; p.f.len_a = d_len_a + s0; p.f.len_b = d_len_b + s0;
      p.f.status = ctx->status.as<uint64_t>() + s0;
      p.f.n_pairs = (uint32_t)m;
      p.score = reinterpret_cast<int32_t *>(d_res + 4) + s0;
      p.pos_a = d_res + 4 + n + s0; p.pos_b = d_res + 4 + 2 * n + s0;
      p.len_a = d_res + 4 + 3 * n + s0; p.len_b = d_res + 4 + 4 * n + s0;
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
        e = sa_launch_span_strips(p, st);
      } else {
        e = sa_launch_span_rows(p, cls_max_a[x], st);
      }
      if (e != hipSuccess) return fail_hip(e, "span kernel launch");
    }
    return SEQALIGN_OK;
  }

  // results home, in pair order; the lowest failing pair of the chunk named
  int finish(uint64_t first, int32_t *out_score, uint32_t *const (&out)[4]) {
    int rc;
    const size_t words = 4 + 5 * n;
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
      return fail_unknown_pair(first + worst);
    }
    const int32_t *hs = reinterpret_cast<const int32_t *>(h + 4);
    constexpr uint64_t kTask = 16384;
    parallel_for((n + kTask - 1) / kTask, [&](uint64_t blk) {
      for (uint64_t s = blk * kTask, e = std::min(n, (blk + 1) * kTask); s < e; ++s) {
        const uint64_t p = first + order[s];
        out_score[p] = hs[s];
        for (int f = 0; f < 4; ++f) out[f][p] = h[4 + (uint64_t)(f + 1) * n + s];
      }
    });
    return SEQALIGN_OK;
  }
};

}  // namespace

extern "C" int seqalign_sw_span_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                      int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a,
                                      uint32_t *out_len_b) {
  if (!ctx || !scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  if (!batch_readable(batch)) return SEQALIGN_E_ARG;   // (no cell cap: the score call's check)
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  int rc;
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, 1, &sc))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  uint32_t *const out[4] = {out_pos_a, out_pos_b, out_len_a, out_len_b};
  for (const SpanChunk &c : plan_span_chunks(batch, ctx->chunk_budget)) {
    SpanChunkRun run;
    run.ctx = ctx; run.sc = sc;
    if ((rc = run.prepare(batch, c)) || (rc = run.launch()) || (rc = run.finish(c.first, out_score, out))) return rc;
  }
  return SEQALIGN_OK;
}

extern "C" int seqalign_sw_span_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                                        float *ms_each) {
  if (!ctx || !scoring || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  if (!batch_readable(batch) || batch->n_pairs == 0) return SEQALIGN_E_ARG;
  const std::vector<SpanChunk> chunks = plan_span_chunks(batch, ctx->chunk_budget);
  if (chunks.size() != 1) { set_last_error("seqalign_sw_span_time_ms: the batch does not fit one chunk"); return SEQALIGN_E_ARG; }
  HIP_TRY(hipSetDevice(ctx->device));
  int rc;
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, 1, &sc))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  SpanChunkRun run;
  run.ctx = ctx; run.sc = sc;
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
