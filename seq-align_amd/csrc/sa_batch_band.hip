// sa_batch_band.hip -- the banded calls over HOST batches: seqalign_nw_score_banded, seqalign_nw_align_banded and the timing
// hook seqalign_band_score_time_ms; seqalign_sw_score_banded, seqalign_sw_align_banded and seqalign_sw_band_score_time_ms;
// seqalign_sw_span_banded and seqalign_sw_span_band_time_ms; seqalign_sw_stats_banded and seqalign_sw_stats_band_time_ms;
// seqalign_nw_stats_banded and seqalign_nw_stats_band_time_ms (the kernels: sa_band.hip, sa_band_span.hip, sa_band_stats.hip,
// sa_band_nw_stats.hip; the contracts: include/seqalign_hip.h).
//
// Everything that can be refused from lengths and bands alone is refused before any device work: the band of every pair is
// clamped to its matrix and a width over SEQALIGN_BAND_MAX_WIDTH is SEQALIGN_E_TOO_LARGE.  Then, per chunk: the pairs are put
// in classes by band WIDTH -- the columns per lane of the one-wave kernels, sa_score_row_class's ladder -- and the
// descriptors laid out class by class, one launch per class; the sequences stay in pair order.  The align call fills M, A, B
// of the band's cells (12 bytes per band cell, (len_b + 1) x width cells per pair), walks all pairs of the chunk in one
// launch and brings home 16 bytes per pair and the strings.
//
// Chunks are cut by device BYTES (header: the bytes per pair); a pair that does not fit the budget alone is
// SEQALIGN_E_NOMEM with the bytes named.  The cut, the staging of a chunk, the lowest failing pair and the timing loop are
// sa_chunks.hpp's; what is here is the band geometry, the kernels' parameters, the wide launch and the align calls' way home.
//
// Banded SW runs through the same chunk plan, layout and launch loop (BandChunkRun::sw).  Its band is the caller's, clipped;
// the align call stores only the rows that have inner band cells (sa_band_sw_rows), the fill reports the best cell, the walk
// brings home 32 bytes per pair (score, status, pos_a, pos_b, end_a, end_b, length, head) and the strings, and the host
// delivers the hits that reach min_score in pair order under seqalign_sw_align_long's capacity rule.
//
// Banded SW hit spans (seqalign_sw_span_banded, seqalign_sw_span_band_time_ms; kernel: sa_band_span.hip) are the SW score
// call's third mode (BandChunkRun::span): its checks with the span cap on the width, its chunk plan, width classes and
// upload; the result record is five words per pair instead of three (finish_span).
//
// Banded SW statistics (seqalign_sw_stats_banded, seqalign_sw_stats_band_time_ms; kernel: sa_band_stats.hip) are the span
// mode with two result words more (BandChunkRun::stats, finish_stats) and sw_stats' length limit checked after the band.
//
// Banded NW statistics (seqalign_nw_stats_banded, seqalign_nw_stats_band_time_ms; kernel: sa_band_nw_stats.hip) are the NW score
// call's second mode (BandChunkRun::nw_stats): its band geometry with the span cap on the width, its chunk plan, width classes
// and upload; three result words per pair instead of one, and a pair whose end value lies below INT32_MIN / 2 -- no alignment
// inside its band -- is SEQALIGN_E_TRACEBACK (finish_nw_stats).
//
// The wide calls (seqalign_*_banded_wide; kernel: sa_band_strips.hip) run through the same plan with a strip width
// (BandChunkRun::wide): no width check, the pipeline's scratch added to a pair's bytes, and per chunk ONE launch over all its
// pairs instead of one per width class; the layouts, the walks and what comes home are the narrow calls'.
#include "sa_chunks.hpp"

using namespace sa_host;

namespace {

constexpr uint64_t kScorePairBytes = 64;   // descriptors (48: the align call's record, mat_off and str_off unused), status (8), score (4), slack
constexpr uint64_t kAlignPairBytes = 96;   // descriptors (48), status (8), the walk's four words (16), slack
constexpr uint64_t kSwScorePairBytes = 80;   // ... and end_a, end_b (8)
constexpr uint64_t kSwSpanPairBytes = 88;    // ... and pos_a, pos_b, len_a, len_b in place of end_a, end_b (16)
constexpr uint64_t kSwStatsPairBytes = 96;   // ... and matches, mismatches behind them (8)
constexpr uint64_t kNwStatsPairBytes = 72;   // descriptors (48), status (8), score, matches, mismatches (12), slack
constexpr uint64_t kSwAlignPairBytes = 128;  // descriptors (48), status (8), score and end cell (12), the walk's eight words (32), slack
// a wide launch has (pairs rounded up to 8) x (the chunk's largest strip count) workgroups, most of which return at once when
// one long pair sits among many short ones: a chunk is cut before that product passes this.  One pair alone stays below it
// (len_a < 2^31, 64 columns per strip at least: fewer than 2^25 strips, times 8)
constexpr uint64_t kWideMaxBlocks = (uint64_t)1 << 28;

struct Band {
  int32_t d_lo;
  uint32_t width;
  uint64_t cells;   // of one matrix in the align call
};

Band band_of(uint32_t la, uint32_t lb, uint32_t w, uint64_t *width64) {
  const int64_t d = (int64_t)la - (int64_t)lb;
  const int64_t d_lo = std::max<int64_t>(-(int64_t)lb, std::min<int64_t>(0, d) - (int64_t)w);
  const int64_t d_hi = std::min<int64_t>((int64_t)la, std::max<int64_t>(0, d) + (int64_t)w);
  *width64 = (uint64_t)(d_hi - d_lo + 1);
  const uint32_t width = (uint32_t)std::min<uint64_t>(*width64, 0xFFFFFFFFu);
  return Band{(int32_t)std::max<int64_t>(d_lo, INT32_MIN), width, ((uint64_t)lb + 1) * width};
}

// banded SW: the caller's bounds clipped to [-len_b, len_a].  A band that is empty then is given to the kernels as the one
// diagonal len_a, which has no inner cell: score 0, nothing stored
Band sw_band_of(uint32_t la, uint32_t lb, int32_t lo, int32_t hi, uint64_t *width64) {
  const int64_t d_lo = std::max<int64_t>(lo, -(int64_t)lb), d_hi = std::min<int64_t>(hi, (int64_t)la);
  if (d_lo > d_hi) { *width64 = 0; return Band{(int32_t)la, 1, 0}; }
  *width64 = (uint64_t)(d_hi - d_lo + 1);
  int64_t j0, j1;
  sa_band_sw_rows(la, lb, d_lo, d_hi, &j0, &j1);
  return Band{(int32_t)d_lo, (uint32_t)std::min<uint64_t>(*width64, 0xFFFFFFFFu), j1 < j0 ? 0 : (uint64_t)(j1 - j0 + 1) * *width64};
}

// the wide calls: a pair's strips of `cols` columns, and what they add to its bytes -- per strip a hand-off column of `width`
// entries of 8 bytes, a progress word (4) and a best-cell entry (16), and per pair two more descriptors (16) and a front word (4)
uint64_t wide_strips(uint32_t la, uint32_t cols) { return la ? ((uint64_t)la + cols - 1) / cols : 1; }
uint64_t wide_bytes(uint32_t la, uint32_t width, uint32_t cols) { return wide_strips(la, cols) * (8 * (uint64_t)width + 20) + 20; }

uint64_t pair_bytes(uint32_t la, uint32_t lb, const Band &g, bool align, bool sw, uint32_t wide_cols, bool span = false,
                    bool stats = false, bool nw_stats = false) {
  const uint64_t seq = (uint64_t)la + lb, cells = g.cells, wide = wide_cols ? wide_bytes(la, g.width, wide_cols) : 0;
  if (nw_stats) return seq + kNwStatsPairBytes;
  if (stats) return seq + kSwStatsPairBytes;
  if (span) return seq + kSwSpanPairBytes;
  if (sw) return wide + (align ? 12 * cells + 3 * seq + kSwAlignPairBytes : seq + kSwScorePairBytes);
  return wide + (align ? 12 * cells + 3 * seq + kAlignPairBytes : seq + kScorePairBytes);
}

// the (pair, strip) waves of a wide launch that sweep at least one row: the strips that hold one of the pair's columns with
// an inner band cell, max(1, 1 + d_lo) .. min(len_a, len_b + d_hi)
uint64_t wide_busy_strips(uint32_t la, uint32_t lb, const Band &g, uint32_t cols) {
  const int64_t d_hi = (int64_t)g.d_lo + g.width - 1;
  const int64_t c_lo = std::max<int64_t>(1, 1 + (int64_t)g.d_lo), c_hi = std::min<int64_t>(la, (int64_t)lb + d_hi);
  if (la == 0 || lb == 0 || c_lo > c_hi) return 0;
  return (uint64_t)((c_hi - 1) / cols - (c_lo - 1) / cols + 1);
}

// columns per strip of a wide call: the option band_strip_cols, or (0) what was fastest where it was measured (DESIGN.md 3.17:
// 512 on both batches of 1 000 pairs, widths 584 and 2 049; 256 on one pair of width 1 023 and on 64 pairs of width 5 653)
uint32_t wide_strip_cols(const seqalign_ctx *ctx, uint64_t n_pairs) {
  if (ctx->opt.band_strip_cols) return ctx->opt.band_strip_cols;
  return n_pairs >= 512 ? 512 : 256;
}

int too_wide(uint64_t p, uint64_t width, uint64_t max_width = SEQALIGN_BAND_MAX_WIDTH) {
  set_last_error("pair " + std::to_string(p) + ": a band of " + std::to_string(width) + " diagonals, at most " +
                 std::to_string(max_width) + " are supported");
  return SEQALIGN_E_TOO_LARGE;
}

int too_long(uint64_t p) {
  set_last_error("pair " + std::to_string(p) + ": len_a + len_b is 2^31 or more");
  return SEQALIGN_E_TOO_LARGE;
}

// argument checks and band geometry, before any device work
int check_band_batch(const seqalign_batch_t *b, const uint32_t *band, std::vector<Band> &geom, bool wide = false,
                     uint64_t max_width = SEQALIGN_BAND_MAX_WIDTH) {
  if (!batch_readable(b)) return SEQALIGN_E_ARG;
  geom.resize(b->n_pairs);
  for (uint64_t p = 0; p < b->n_pairs; ++p) {
    const uint32_t la = b->len_a[p], lb = b->len_b[p];
    if ((uint64_t)la + lb >= ((uint64_t)1 << 31)) return too_long(p);
    uint64_t width = 0;
    geom[p] = band_of(la, lb, band[p], &width);
    if (!wide && width > max_width) return too_wide(p, width, max_width);
  }
  return SEQALIGN_OK;
}

// ... of the banded SW calls (max_width: the score and align calls' cap, or the span call's)
int check_sw_band_batch(const seqalign_batch_t *b, const int32_t *diag_lo, const int32_t *diag_hi, std::vector<Band> &geom, bool wide = false,
                        uint64_t max_width = SEQALIGN_BAND_MAX_WIDTH) {
  if (!batch_readable(b)) return SEQALIGN_E_ARG;
  geom.resize(b->n_pairs);
  for (uint64_t p = 0; p < b->n_pairs; ++p) {
    const uint32_t la = b->len_a[p], lb = b->len_b[p];
    if (diag_lo[p] > diag_hi[p]) {
      set_last_error("pair " + std::to_string(p) + ": diag_lo " + std::to_string(diag_lo[p]) + " is above diag_hi " + std::to_string(diag_hi[p]));
      return SEQALIGN_E_ARG;
    }
    if ((uint64_t)la + lb >= ((uint64_t)1 << 31)) return too_long(p);
    uint64_t width = 0;
    geom[p] = sw_band_of(la, lb, diag_lo[p], diag_hi[p], &width);
    if (!wide && width > max_width) return too_wide(p, width, max_width);
  }
  return SEQALIGN_OK;
}

// cut_chunks with the banded calls' bytes per pair, the band cells summed per chunk and the wide launch's grid capped
int plan_band_chunks(const seqalign_batch_t *b, const std::vector<Band> &geom, bool align, bool sw, size_t budget, std::vector<ByteChunk> &out,
                     uint32_t wide_cols = 0, bool span = false, bool stats = false, bool nw_stats = false) {
  return cut_chunks(b, budget, [&](uint64_t p) {
    const uint32_t la = b->len_a[p];
    return PairNeed{pair_bytes(la, b->len_b[p], geom[p], align, sw, wide_cols, span, stats, nw_stats), geom[p].cells, wide_cols ? wide_strips(la, wide_cols) : 0};
  }, out, true, kWideMaxBlocks);
}

// One chunk laid out and uploaded; launch() enqueues its kernels on ctx->stream
struct BandChunkRun {
  seqalign_ctx *ctx = nullptr;
  const seqalign_dev_scoring *sc = nullptr;
  bool align = false, sw = false;
  bool span = false;                                    // banded SW hit spans: sw, not align, not wide
  bool stats = false;                                   // banded SW statistics: span, and two result words more
  bool nw_stats = false;                                // banded NW statistics: not sw, not align, not wide
  // classes by band width; the descriptors behind the shared ones: mat_off, str_off (wide: slot_off, hand_off), width, d_lo
  ChunkStage<SA_SCORE_ROW_CLASSES> stage;
  uint64_t n = 0, seq_bytes = 0;
  uint32_t *d_res = nullptr;                            // [4] header (err_flag; wide: give-up word), then score[n]; SW: end_a[n], end_b[n] behind it
                                                        // (span: pos_a[n], pos_b[n], len_a[n], len_b[n]; stats: matches[n],
                                                        // mismatches[n] behind those); nw_stats: matches[n], mismatches[n]
  uint64_t cells = 0;
  // the wide calls: columns per strip (0: the narrow calls), one launch per chunk over all its slots
  uint32_t wide = 0, strips_per_pair = 0;
  uint64_t slots = 0, hand_total = 0, busy_strips = 0;

  BandChunkRun(seqalign_ctx *c, const seqalign_dev_scoring *scoring, bool align_, bool sw_, uint32_t wide_cols, bool span_ = false,
               bool stats_ = false, bool nw_stats_ = false)
      : ctx(c), sc(scoring), align(align_), sw(sw_), span(span_), stats(stats_), nw_stats(nw_stats_), wide(wide_cols) { stage.ctx = c; }

  // slot -> where its strings start in the chunk's string buffers: where its sequences do (a pair's strings are len_a + len_b
  // bytes at most); read from the pinned descriptors, which stay as laid out until the next chunk
  uint64_t str_at(uint64_t s) const { return stage.h_off_a[s]; }

  int prepare(const seqalign_batch_t *b, const std::vector<Band> &geom, const ByteChunk &c) {
    int rc;
    n = c.count; seq_bytes = c.seq_bytes; cells = c.cells;
    slots = hand_total = busy_strips = 0; strips_per_pair = 0;
    uint64_t mat = 0;
    rc = stage.lay_out(b, c, sa_score_row_class, [&](uint64_t p) { return geom[p].width; }, wide ? 4 : 2, 2, [&](uint64_t s, uint64_t p) {
      const uint32_t la = b->len_a[p], lb = b->len_b[p];
      stage.h_u32(0)[s] = geom[p].width; stage.h_u32<int32_t>(1)[s] = geom[p].d_lo;
      stage.h_u64(0)[s] = mat; mat += geom[p].cells;
      stage.h_u64(1)[s] = str_at(s);
      if (wide) {
        const uint64_t strips = wide_strips(la, wide);
        stage.h_u64(2)[s] = slots; stage.h_u64(3)[s] = hand_total;
        slots += strips; hand_total += strips * geom[p].width;
        strips_per_pair = (uint32_t)std::max<uint64_t>(strips_per_pair, strips);
        busy_strips += wide_busy_strips(la, lb, geom[p], wide);
      }
    });
    if (rc || (rc = ctx->best_score.reserve(16 + (stats ? 28 : span ? 20 : (sw || nw_stats) ? 12 : 4) * n))) return rc;
    if (align && ((rc = ctx->long_block.reserve(12 * cells + 64)) || (rc = ctx->t_out_a.reserve(seq_bytes + 16)) ||
                  (rc = ctx->t_out_b.reserve(seq_bytes + 16)) || (rc = ctx->t_meta.reserve((sw ? 32 : 16) * n))))
      return rc;
    // wide: progress words, the ticket counter and the pairs' front words behind them, then (16-byte aligned) the best-cell
    // entries; the hand-off columns
    if (wide && ((rc = ctx->strip_progress.reserve(4 * (slots + n + 8) + 16 * slots + 16)) || (rc = ctx->score_handoff.reserve(8 * hand_total + 16))))
      return rc;
    d_res = ctx->best_score.as<uint32_t>();
    return stage.upload();
  }

  SaBandParams params(uint64_t s0, uint64_t m) const {
    SaBandParams p;
    memset(&p, 0, sizeof(p));
    p.f = score_fill_params(sc);
    stage.set_slots(p.f, s0, m);
    p.f.mat_off = stage.d_u64(0) + s0;
    p.d_lo = stage.d_u32<int32_t>(1) + s0; p.width = stage.d_u32(0) + s0;
    p.score = reinterpret_cast<int32_t *>(d_res + 4) + s0;
    p.err_flag = d_res;
    if (align) {
      p.f.M = ctx->long_block.as<int32_t>(); p.f.A = p.f.M + cells; p.f.B = p.f.A + cells;
      p.str_off = stage.d_u64(1) + s0;
      p.out_a = ctx->t_out_a.as<char>(); p.out_b = ctx->t_out_b.as<char>();
      p.meta4 = ctx->t_meta.as<uint32_t>() + 4 * s0;
    }
    return p;
  }

  SaBandSwParams sw_params(uint64_t s0, uint64_t m) const {
    SaBandSwParams p;
    p.b = params(s0, m);
    p.b.meta4 = nullptr;
    p.end_a = d_res + 4 + n + s0; p.end_b = d_res + 4 + 2 * n + s0;
    p.meta8 = align ? ctx->t_meta.as<uint32_t>() + 8 * s0 : nullptr;
    return p;
  }

  SaBandSpanParams span_params(uint64_t s0, uint64_t m) const {
    SaBandSpanParams p;
    p.b = params(s0, m);
    p.pos_a = d_res + 4 + n + s0; p.pos_b = d_res + 4 + 2 * n + s0;
    p.len_a = d_res + 4 + 3 * n + s0; p.len_b = d_res + 4 + 4 * n + s0;
    return p;
  }

  // seven result arrays behind the 16-byte header: the span call's five, then matches and mismatches
  SaBandSwStatsParams stats_params(uint64_t s0, uint64_t m) const {
    SaBandSwStatsParams p;
    p.b = params(s0, m);
    p.pos_a = d_res + 4 + n + s0; p.pos_b = d_res + 4 + 2 * n + s0;
    p.len_a = d_res + 4 + 3 * n + s0; p.len_b = d_res + 4 + 4 * n + s0;
    p.matches = d_res + 4 + 5 * n + s0; p.mismatches = d_res + 4 + 6 * n + s0;
    return p;
  }

  // banded NW statistics: matches and mismatches behind the score
  SaBandNwStatsParams nw_stats_params(uint64_t s0, uint64_t m) const {
    SaBandNwStatsParams p;
    p.b = params(s0, m);
    p.matches = d_res + 4 + n + s0; p.mismatches = d_res + 4 + 2 * n + s0;
    return p;
  }

  // the wide calls: one launch over all slots of the chunk, strips_per_pair the chunk's maximum
  int launch_wide() {
    hipStream_t st = ctx->stream;
    SaBandStripsParams w;
    memset(&w, 0, sizeof(w));
    w.s = sw_params(0, n);
    if (!sw) { w.s.b = params(0, n); w.s.end_a = w.s.end_b = w.s.meta8 = nullptr; }
    w.strips_per_pair = strips_per_pair;
    w.slot_off = stage.d_u64(2); w.hand_off = stage.d_u64(3);
    w.progress = ctx->strip_progress.as<uint32_t>();
    w.ticket = w.progress + slots;
    w.front = w.ticket + 1;
    w.strip_best = w.progress + ((slots + n + 4) & ~(uint64_t)3);
    w.give_up = d_res + 1;
    w.handoff = ctx->score_handoff.as<int32_t>();
    HIP_TRY(hipMemsetAsync(w.progress, 0, 4 * (slots + 1 + n), st));
    HIP_TRY(hipMemsetAsync(ctx->status.p, 0xFF, 8 * n, st));
    const hipError_t e = sa_launch_band_strips(w, wide, align, sw, busy_strips, st);
    if (e != hipSuccess) return fail_hip(e, "band strips kernel launch");
    return SEQALIGN_OK;
  }

  // wide: the give-up word of the header brought home in h (finish_*): slot + 1 of the first pair one of whose strips gave up
  int fail_if_gave_up(const uint32_t *h) {
    if (!wide || !h[1]) return SEQALIGN_OK;
    const uint64_t slot = h[1] - 1;
    set_last_error("pair " + std::to_string(stage.first + (slot < n ? stage.order[slot] : 0)) + ": band strip hand-off timed out");
    return SEQALIGN_E_HIP;
  }

  // wide align calls: the header on its way home with the walk's results (the narrow calls have no give-up word)
  int fetch_give_up() {
    if (!wide) return SEQALIGN_OK;
    int rc = ctx->h_misc.reserve(16);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->h_misc.p, d_res, 16, hipMemcpyDeviceToHost, ctx->stream));
    return SEQALIGN_OK;
  }

  int launch() {
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemsetAsync(d_res, 0, 16, st));
    if (wide) {
      int rc = launch_wide();
      if (rc) return rc;
    }
    for (int x = 0; x < SA_SCORE_ROW_CLASSES && !wide; ++x) {
      const uint64_t s0 = stage.cls_first[x], m = stage.class_size(x);
      if (!m) continue;
      hipError_t e;
      if (nw_stats) {
        e = sa_launch_band_nw_stats(nw_stats_params(s0, m), stage.cls_max[x], st);
      } else if (stats) {
        e = sa_launch_band_sw_stats(stats_params(s0, m), stage.cls_max[x], st);
      } else if (span) {
        e = sa_launch_band_span(span_params(s0, m), stage.cls_max[x], st);
      } else if (sw) {
        const SaBandSwParams p = sw_params(s0, m);
        e = align ? sa_launch_band_sw_fill(p, stage.cls_max[x], st) : sa_launch_band_sw_score(p, stage.cls_max[x], st);
      } else {
        const SaBandParams p = params(s0, m);
        e = align ? sa_launch_band_fill(p, stage.cls_max[x], st) : sa_launch_band_score(p, stage.cls_max[x], st);
      }
      if (e != hipSuccess) return fail_hip(e, "band kernel launch");
    }
    if (align) {
      const hipError_t e = sw ? sa_launch_band_sw_walk(sw_params(0, n), st) : sa_launch_band_walk(params(0, n), st);
      if (e != hipSuccess) return fail_hip(e, "band walk launch");
    }
    return SEQALIGN_OK;
  }

  // the score calls: score per pair, banded SW: end_a and end_b behind it; the lowest pair of the chunk whose fill met a band
  // cell without a score named
  int finish_score(int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b) {
    int rc;
    const int fields = sw ? 3 : 1;
    const size_t words = 4 + fields * n;
    if ((rc = ctx->h_misc.reserve(4 * words))) return rc;
    uint32_t *h = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h, d_res, 4 * words, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    if ((rc = fail_if_gave_up(h))) return rc;
    if (h[0]) return stage.fail_from_status();
    uint32_t *const out[2] = {out_end_a, out_end_b};
    stage.scatter(h + 4, fields, out_score, out);
    return SEQALIGN_OK;
  }

  // the span call: five fields per pair through the stage's order, as finish_score scatters three
  int finish_span(int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b) {
    int rc;
    const size_t words = 4 + 5 * n;
    if ((rc = ctx->h_misc.reserve(4 * words))) return rc;
    uint32_t *h = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h, d_res, 4 * words, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    if (h[0]) return stage.fail_from_status();
    uint32_t *const out[4] = {out_pos_a, out_pos_b, out_len_a, out_len_b};
    stage.scatter(h + 4, 5, out_score, out);
    return SEQALIGN_OK;
  }

  // the statistics call: seven fields per pair, as finish_span scatters five
  int finish_stats(int32_t *out_score, uint32_t *const (&out)[6]) {
    int rc;
    const size_t words = 4 + 7 * n;
    if ((rc = ctx->h_misc.reserve(4 * words))) return rc;
    uint32_t *h = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h, d_res, 4 * words, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    if (h[0]) return stage.fail_from_status();
    stage.scatter(h + 4, 7, out_score, out);
    return SEQALIGN_OK;
  }

  // banded NW statistics: three fields per pair.  A pair whose end value lies below INT32_MIN / 2 has no alignment inside its
  // band: SEQALIGN_E_TRACEBACK, decided by the value (include/seqalign_hip.h).  Between it and a pair without a score the
  // lower pair's code is the call's, as in seqalign_nw_stats_batch
  int finish_nw_stats(int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches) {
    int rc;
    const size_t words = 4 + 3 * n;
    if ((rc = ctx->h_misc.reserve(4 * words))) return rc;
    uint32_t *h = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h, d_res, 4 * words, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    uint64_t unknown = ~0ull, no_walk = ~0ull;   // the chunk's lowest failing pairs, as batch indices
    if (h[0] && (rc = stage.fail_from_status(&unknown)) != SEQALIGN_E_UNKNOWN_PAIR) return rc;
    const int32_t *hs = reinterpret_cast<const int32_t *>(h + 4);
    for (uint64_t s = 0; s < n; ++s)
      if (hs[s] < INT32_MIN / 2) no_walk = std::min<uint64_t>(no_walk, stage.first + stage.order[s]);
    if (no_walk < unknown) {
      set_last_error("pair " + std::to_string(no_walk) + ": traceback failed (no alignment inside the band)");
      return SEQALIGN_E_TRACEBACK;
    }
    if (h[0]) return SEQALIGN_E_UNKNOWN_PAIR;
    uint32_t *const out[2] = {out_matches, out_mismatches};
    stage.scatter(h + 4, 3, out_score, out);
    return SEQALIGN_OK;
  }

  // banded SW: the chunk's hits in pair order, under seqalign_sw_align_long's capacity rule.  A pair's own error comes before
  // SEQALIGN_E_NOMEM and nothing of the chunk is delivered then.
  int finish_sw_align(const int32_t *min_score, seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits,
                      char *out_a, char *out_b, uint64_t str_cap, uint64_t *used_str) {
    int rc;
    const uint64_t first = stage.first;
    const std::vector<uint32_t> &order = stage.order;
    if ((rc = ctx->h_tmeta.reserve(32 * n)) || (rc = ctx->h_ta.reserve(seq_bytes + 16)) || (rc = ctx->h_tb.reserve(seq_bytes + 16))) return rc;
    hipStream_t st = ctx->stream;
    const uint32_t *meta = ctx->h_tmeta.as<uint32_t>();
    if ((rc = fetch_give_up())) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->h_tmeta.p, ctx->t_meta.p, 32 * n, hipMemcpyDeviceToHost, st));
    if (seq_bytes) {
      HIP_TRY(hipMemcpyAsync(ctx->h_ta.p, ctx->t_out_a.p, seq_bytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(ctx->h_tb.p, ctx->t_out_b.p, seq_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(stream_wait_spinning(st));
    if (wide && (rc = fail_if_gave_up(ctx->h_misc.as<uint32_t>()))) return rc;
    std::vector<uint32_t> slot_of(n);
    uint64_t worst = ~0ull;
    uint32_t worst_code = 0;
    for (uint64_t s = 0; s < n; ++s) {
      slot_of[order[s]] = (uint32_t)s;
      if (meta[8 * s + 1] && order[s] < worst) { worst = order[s]; worst_code = meta[8 * s + 1]; }
    }
    if (worst != ~0ull) {
      if (worst_code == SEQALIGN_E_UNKNOWN_PAIR) return fail_unknown_pair(first + worst);
      set_last_error("pair " + std::to_string(first + worst) + ": traceback failed");
      return (int)worst_code;
    }
    const char *ha = ctx->h_ta.as<char>(), *hb = ctx->h_tb.as<char>();
    for (uint64_t k = 0; k < n; ++k) {
      const uint64_t s = slot_of[k], p = first + k;
      const uint32_t *m = meta + 8 * s;
      const int32_t score = (int32_t)m[0];
      if (score <= 0 || score < min_score[p]) continue;   // no hit
      const uint32_t len = m[6], head = m[7];
      const uint64_t took = *n_hits >= hit_cap ? 0 : put_alignment(ctx, ha + str_at(s) + head, hb + str_at(s) + head, len, out_a, out_b, *used_str,
                                                                    str_cap > *used_str ? str_cap - *used_str : 0);
      if (!took) return SEQALIGN_E_NOMEM;
      seqalign_sw_hit_t &h = hits[(*n_hits)++];
      h.pair = p; h.score = score;
      h.pos_a = m[2]; h.pos_b = m[3]; h.len_a = m[4] - m[2]; h.len_b = m[5] - m[3];   // smith_waterman.c:251-255
      h.length = len; h.str_off = *used_str;
      *used_str += took;
    }
    return SEQALIGN_OK;
  }

  int finish_align(const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score) {
    int rc;
    const uint64_t first = stage.first;
    const std::vector<uint32_t> &order = stage.order;
    if ((rc = ctx->h_tmeta.reserve(16 * n)) || (rc = ctx->h_ta.reserve(seq_bytes + 16)) || (rc = ctx->h_tb.reserve(seq_bytes + 16))) return rc;
    hipStream_t st = ctx->stream;
    uint32_t *meta = ctx->h_tmeta.as<uint32_t>();
    if ((rc = fetch_give_up())) return rc;
    HIP_TRY(hipMemcpyAsync(meta, ctx->t_meta.p, 16 * n, hipMemcpyDeviceToHost, st));
    if (seq_bytes) {
      HIP_TRY(hipMemcpyAsync(ctx->h_ta.p, ctx->t_out_a.p, seq_bytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(ctx->h_tb.p, ctx->t_out_b.p, seq_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(stream_wait_spinning(st));
    if (wide && (rc = fail_if_gave_up(ctx->h_misc.as<uint32_t>()))) return rc;
    uint64_t worst = ~0ull;
    uint32_t worst_code = 0;
    for (uint64_t s = 0; s < n; ++s)
      if (meta[4 * s + 3] && order[s] < worst) { worst = order[s]; worst_code = meta[4 * s + 3]; }
    if (worst != ~0ull) {
      if (worst_code == SEQALIGN_E_UNKNOWN_PAIR) return fail_unknown_pair(first + worst);
      set_last_error("pair " + std::to_string(first + worst) + ": traceback failed (no alignment inside the band)");
      return (int)worst_code;
    }
    const char *ha = ctx->h_ta.as<char>(), *hb = ctx->h_tb.as<char>();
    constexpr uint64_t kTask = 64;
    parallel_for((n + kTask - 1) / kTask, [&](uint64_t blk) {
      for (uint64_t s = blk * kTask, e = std::min(n, (blk + 1) * kTask); s < e; ++s) {
        const uint64_t p = first + order[s];
        const uint32_t head = meta[4 * s], len = meta[4 * s + 1];
        memcpy(out_a + str_off[p], ha + str_at(s) + head, len);
        memcpy(out_b + str_off[p], hb + str_at(s) + head, len);
        out_a[str_off[p] + len] = out_b[str_off[p] + len] = '\0';
        out_len[p] = len;
        out_score[p] = (int32_t)meta[4 * s + 2];
      }
    });
    return SEQALIGN_OK;
  }
};

// A banded call behind its checks: every chunk prepared, launched and brought home by finish(run)
template <class Finish>
int band_call(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const std::vector<Band> &geom, bool align, bool sw,
              bool wide, Finish finish, bool span = false, bool stats = false, bool nw_stats = false) {
  int rc;
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, sw ? 1 : 0, &sc))) return rc;
  if ((rc = admit_batch(sc, batch, SA_FRAMES_BAND))) return rc;
  std::vector<ByteChunk> chunks;
  const uint32_t cols = wide ? wide_strip_cols(ctx, batch->n_pairs) : 0;
  if ((rc = plan_band_chunks(batch, geom, align, sw, ctx->chunk_budget, chunks, cols, span, stats, nw_stats))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  for (const ByteChunk &c : chunks) {
    BandChunkRun run(ctx, sc, align, sw, cols, span, stats, nw_stats);
    if ((rc = run.prepare(batch, geom, c)) || (rc = run.launch()) || (rc = finish(run))) return rc;
  }
  return SEQALIGN_OK;
}

// the score call's (span: the span call's, stats / nw_stats: the statistics calls') launches of one chunk, `repeats` times between HIP events
int band_time(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const std::vector<Band> &geom, bool sw,
              int repeats, float *ms_each, const char *name, bool span = false, bool stats = false, bool nw_stats = false) {
  int rc;
  if (batch->n_pairs == 0) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, sw ? 1 : 0, &sc))) return rc;
  if ((rc = admit_batch(sc, batch, SA_FRAMES_BAND))) return rc;
  std::vector<ByteChunk> chunks;
  if ((rc = plan_band_chunks(batch, geom, false, sw, ctx->chunk_budget, chunks, 0, span, stats, nw_stats))) return rc;
  if (chunks.size() != 1) { set_last_error(std::string(name) + ": the batch does not fit one chunk"); return SEQALIGN_E_ARG; }
  StreamSyncOnExit sync(ctx->stream);
  BandChunkRun run(ctx, sc, false, sw, 0, span, stats, nw_stats);
  if ((rc = run.prepare(batch, geom, chunks[0]))) return rc;
  return time_launches(ctx->stream, repeats, ms_each, [&] { return run.launch(); });
}

// ---- the four contracts, each the body of its narrow call and of its wide one (any width; kernel: sa_band_strips.hip)
int nw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const uint32_t *band, int32_t *out_score,
                    bool wide) {
  if (!ctx || !batch || !scoring || !band || !out_score) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch(batch, band, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  return band_call(ctx, batch, scoring, geom, false, false, wide, [&](BandChunkRun &run) { return run.finish_score(out_score, nullptr, nullptr); });
}

int nw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const uint32_t *band, const uint64_t *str_off,
                    char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score, bool wide) {
  if (!ctx || !batch || !scoring || !band || !str_off || !out_a || !out_b || !out_len || !out_score) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch(batch, band, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  return band_call(ctx, batch, scoring, geom, true, false, wide,
                   [&](BandChunkRun &run) { return run.finish_align(str_off, out_a, out_b, out_len, out_score); });
}

int sw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo, const int32_t *diag_hi,
                    int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_end_a || !out_end_b) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_band_batch(batch, diag_lo, diag_hi, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  return band_call(ctx, batch, scoring, geom, false, true, wide, [&](BandChunkRun &run) { return run.finish_score(out_score, out_end_a, out_end_b); });
}

int sw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo, const int32_t *diag_hi,
                    const int32_t *min_score, seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b,
                    uint64_t str_cap, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !min_score || !hits || !n_hits || !out_a || !out_b) return SEQALIGN_E_ARG;
  *n_hits = 0;
  std::vector<Band> geom;
  int rc = check_sw_band_batch(batch, diag_lo, diag_hi, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint64_t used_str = 0;
  return band_call(ctx, batch, scoring, geom, true, true, wide, [&](BandChunkRun &run) {
    return run.finish_sw_align(min_score, hits, hit_cap, n_hits, out_a, out_b, str_cap, &used_str);
  });
}

}  // namespace

extern "C" int seqalign_nw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const uint32_t *band, int32_t *out_score) {
  return nw_score_banded(ctx, batch, scoring, band, out_score, false);
}

extern "C" int seqalign_nw_score_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const uint32_t *band, int32_t *out_score) {
  return nw_score_banded(ctx, batch, scoring, band, out_score, true);
}

extern "C" int seqalign_band_score_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                           const uint32_t *band, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !band || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch(batch, band, geom);
  if (rc) return rc;
  return band_time(ctx, batch, scoring, geom, false, repeats, ms_each, "seqalign_band_score_time_ms");
}

extern "C" int seqalign_nw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const uint32_t *band, const uint64_t *str_off, char *out_a, char *out_b,
                                        uint32_t *out_len, int32_t *out_score) {
  return nw_align_banded(ctx, batch, scoring, band, str_off, out_a, out_b, out_len, out_score, false);
}

extern "C" int seqalign_nw_align_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const uint32_t *band, const uint64_t *str_off, char *out_a, char *out_b,
                                             uint32_t *out_len, int32_t *out_score) {
  return nw_align_banded(ctx, batch, scoring, band, str_off, out_a, out_b, out_len, out_score, true);
}

extern "C" int seqalign_sw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                                        uint32_t *out_end_b) {
  return sw_score_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_end_a, out_end_b, false);
}

extern "C" int seqalign_sw_score_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                                             uint32_t *out_end_b) {
  return sw_score_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_end_a, out_end_b, true);
}

extern "C" int seqalign_sw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const int32_t *diag_lo, const int32_t *diag_hi, const int32_t *min_score,
                                        seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b,
                                        uint64_t str_cap) {
  return sw_align_banded(ctx, batch, scoring, diag_lo, diag_hi, min_score, hits, hit_cap, n_hits, out_a, out_b, str_cap, false);
}

extern "C" int seqalign_sw_align_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const int32_t *diag_lo, const int32_t *diag_hi, const int32_t *min_score,
                                             seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b,
                                             uint64_t str_cap) {
  return sw_align_banded(ctx, batch, scoring, diag_lo, diag_hi, min_score, hits, hit_cap, n_hits, out_a, out_b, str_cap, true);
}

extern "C" int seqalign_sw_span_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a,
                                       uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_band_batch(batch, diag_lo, diag_hi, geom, false, SEQALIGN_SPAN_BAND_MAX_WIDTH);
  if (rc) return rc;
  CallScope scope(ctx);
  return band_call(ctx, batch, scoring, geom, false, true, false,
                   [&](BandChunkRun &run) { return run.finish_span(out_score, out_pos_a, out_pos_b, out_len_a, out_len_b); }, true);
}

extern "C" int seqalign_sw_span_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_band_batch(batch, diag_lo, diag_hi, geom, false, SEQALIGN_SPAN_BAND_MAX_WIDTH);
  if (rc) return rc;
  return band_time(ctx, batch, scoring, geom, true, repeats, ms_each, "seqalign_sw_span_band_time_ms", true);
}

// the statistics calls' checks in the header's order: the band (with the span cap on the width), then sw_stats' length limit
static int check_sw_stats_band_batch(const seqalign_batch_t *batch, const int32_t *diag_lo, const int32_t *diag_hi, std::vector<Band> &geom) {
  const int rc = check_sw_band_batch(batch, diag_lo, diag_hi, geom, false, SEQALIGN_SPAN_BAND_MAX_WIDTH);
  return rc ? rc : sw_stats_check_batch(batch);
}

extern "C" int seqalign_sw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a,
                                        uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b, uint32_t *out_matches,
                                        uint32_t *out_mismatches) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b ||
      !out_matches || !out_mismatches)
    return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_stats_band_batch(batch, diag_lo, diag_hi, geom);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[6] = {out_pos_a, out_pos_b, out_len_a, out_len_b, out_matches, out_mismatches};
  return band_call(ctx, batch, scoring, geom, false, true, false, [&](BandChunkRun &run) { return run.finish_stats(out_score, out); }, true, true);
}

extern "C" int seqalign_sw_stats_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_stats_band_batch(batch, diag_lo, diag_hi, geom);
  if (rc) return rc;
  return band_time(ctx, batch, scoring, geom, true, repeats, ms_each, "seqalign_sw_stats_band_time_ms", true, true);
}

// banded NW statistics: seqalign_nw_score_banded's checks in its order, with the span cap on the width
extern "C" int seqalign_nw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const uint32_t *band, int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches) {
  if (!ctx || !batch || !scoring || !band || !out_score || !out_matches || !out_mismatches) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch(batch, band, geom, false, SEQALIGN_SPAN_BAND_MAX_WIDTH);
  if (rc) return rc;
  CallScope scope(ctx);
  return band_call(ctx, batch, scoring, geom, false, false, false,
                   [&](BandChunkRun &run) { return run.finish_nw_stats(out_score, out_matches, out_mismatches); }, false, false, true);
}

extern "C" int seqalign_nw_stats_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const uint32_t *band, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !band || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch(batch, band, geom, false, SEQALIGN_SPAN_BAND_MAX_WIDTH);
  if (rc) return rc;
  return band_time(ctx, batch, scoring, geom, false, repeats, ms_each, "seqalign_nw_stats_band_time_ms", false, false, true);
}

extern "C" int seqalign_sw_band_score_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_band_batch(batch, diag_lo, diag_hi, geom);
  if (rc) return rc;
  return band_time(ctx, batch, scoring, geom, true, repeats, ms_each, "seqalign_sw_band_score_time_ms");
}
