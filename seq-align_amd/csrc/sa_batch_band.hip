// sa_batch_band.hip -- the banded calls over HOST batches: the twenty-eight seqalign_*_banded, *_banded_wide and *_band_time_ms entry
// points (the contracts: include/seqalign_hip.h; the kernels: sa_band.hip, sa_band_span.hip, sa_band_stats.hip, sa_band_counts.hip, sa_band_gaps.hip,
// sa_band_nw_stats.hip, sa_band_strips.hip, sa_band_nw_stats_strips.hip, sa_band_nw_gaps.hip).  DESIGN.md 3.23b.
//
// One driver, ten modes.  A mode is a traits struct (below): NW or SW, score family or align, its result words and fixed
// bytes per pair, its cap on the width, its kernels' parameter block and launches.  The driver is the same for all of them:
//   checks   everything that can be refused from lengths and bands alone is refused before any device work
//            (check_band_batch): the band of every pair is clipped to its matrix -- NW: w diagonals around the corner cells'
//            (NwBands); SW: the caller's two bounds (SwBands) -- and a width over the mode's cap is SEQALIGN_E_TOO_LARGE.
//   chunks   cut by device BYTES (pair_bytes; the header names them); a pair that does not fit the budget alone is
//            SEQALIGN_E_NOMEM with the bytes named.
//   a chunk  (BandChunkRun) its pairs put in classes by band WIDTH -- the columns per lane of the one-wave kernels,
//            sa_score_row_class's ladder -- the descriptors laid out class by class, one launch per class; the sequences stay
//            in pair order.  An align mode fills M, A, B of the band's cells (12 bytes per cell; NW: (len_b + 1) x width cells
//            per pair, SW: only the rows with inner band cells, sa_band_sw_rows) and walks all pairs of the chunk in one launch.
//   home     the score family: a header and the mode's result arrays, scattered into the caller's in pair order
//            (finish_words).  NW align: 16 bytes per pair and the strings, copied to the caller's offsets (finish_align).  SW
//            align: 32 bytes per pair (score, status, pos_a, pos_b, end_a, end_b, length, head) and the strings; the hits that
//            reach min_score are delivered in pair order under seqalign_sw_align_long's capacity rule (finish_sw_align).
// The cut, the staging of a chunk, the lowest failing pair and the timing loop are sa_chunks.hpp's.
//
// The wide calls (every mode has one) run through the same plan with a strip width (BandChunkRun::wide, a runtime value):
// no width check, the pipeline's scratch added to a pair's bytes, and per chunk ONE launch over all its pairs instead of one
// per width class; the layouts, the walks and what comes home are the narrow calls'.
#include "sa_chunks.hpp"

using namespace sa_host;

namespace {

// ---- the modes.  Of each: kSw (the SW recurrence and scoring), kAlign (fills M/A/B and walks), kFields (result words per pair
// behind the header: the score first), kPairBytes (the fixed bytes per pair the chunk cut counts: descriptors (48), status (8),
// the result words, kAlign: the walk's words; slack), kMaxWidth (the narrow call's cap),
// Params with base() (its SaBandParams), set_results() (the arrays behind the score, res = the score's, n words each) and
// launch() (one width class; recorded as band_score or band_fill).  The score family besides: kMarkField (above 0: the result
// array whose words carry SA_STATS_NO_WALK, SEQALIGN_E_TRACEBACK).  The align modes: the walk's record per pair in words, where its status sits, what
// their message adds to "traceback failed", set_meta() and walk().  The wide form of each: kHandoffBytes (per entry of a
// strip's hand-off column), kBestBytes (per strip: its best-cell entry) and launch_strips() (one launch over a chunk's strips, laid out as SaBandStripsLayout says: sa_kernels.h, where a wide launch finds its pipeline's words).

// the four score and align modes: band_strips_kernel (sa_band_strips.hip), 8 bytes per hand-off entry
hipError_t launch_score_strips(const SaBandSwParams &s, const SaBandStripsLayout &l, uint32_t cols, bool fill, bool is_sw, uint64_t items, hipStream_t st) {
  return sa_launch_band_strips({s, l}, cols, fill, is_sw, items, st);
}

struct NwScoreBand {   // seqalign_nw_score_banded(_wide), seqalign_band_score_time_ms
  using Params = SaBandParams;
  static constexpr bool kSw = false, kAlign = false;
  static constexpr int kFields = 1;             // score
  static constexpr int kMarkField = 0;          // no result word carries a mark
  static constexpr uint64_t kPairBytes = 64, kMaxWidth = SEQALIGN_BAND_MAX_WIDTH, kHandoffBytes = 8, kBestBytes = 16;
  static SaBandParams &base(Params &p) { return p; }
  static void set_results(Params &, uint32_t *, uint64_t) {}
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_score(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    SaBandSwParams s{}; s.b = p;
    return launch_score_strips(s, l, cols, kAlign, kSw, items, st);
  }
};

struct NwAlignBand {   // seqalign_nw_align_banded(_wide)
  using Params = SaBandParams;
  static constexpr bool kSw = false, kAlign = true;
  static constexpr int kFields = 1;
  static constexpr uint64_t kPairBytes = 96, kMaxWidth = SEQALIGN_BAND_MAX_WIDTH, kHandoffBytes = 8, kBestBytes = 16;   // the walk's four words (16)
  static constexpr int kMetaWords = 4, kMetaStatus = 3;   // head, length, score, status
  static constexpr const char *kNoWalkText = " (no alignment inside the band)";
  static SaBandParams &base(Params &p) { return p; }
  static void set_results(Params &, uint32_t *, uint64_t) {}
  static void set_meta(Params &p, uint32_t *meta, uint64_t s0) { p.meta4 = meta + 4 * s0; }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_fill(p, max_width, st); }
  static hipError_t walk(const Params &p, hipStream_t st) { return sa_launch_band_walk(p, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    SaBandSwParams s{}; s.b = p;
    return launch_score_strips(s, l, cols, kAlign, kSw, items, st);
  }
};

struct SwScoreBand {   // seqalign_sw_score_banded(_wide), seqalign_sw_band_score_time_ms
  using Params = SaBandSwParams;
  static constexpr bool kSw = true, kAlign = false;
  static constexpr int kFields = 3;             // score, end_a, end_b
  static constexpr int kMarkField = 0;
  static constexpr uint64_t kPairBytes = 80, kMaxWidth = SEQALIGN_BAND_MAX_WIDTH, kHandoffBytes = 8, kBestBytes = 16;
  static SaBandParams &base(Params &p) { return p.b; }
  static void set_results(Params &p, uint32_t *res, uint64_t n) { p.end_a = res + n; p.end_b = res + 2 * n; }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_sw_score(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return launch_score_strips(p, l, cols, kAlign, kSw, items, st);
  }
};

struct SwAlignBand {   // seqalign_sw_align_banded(_wide)
  using Params = SaBandSwParams;
  static constexpr bool kSw = true, kAlign = true;
  static constexpr int kFields = 3;             // the fill's best cell: score, end_a, end_b
  static constexpr uint64_t kPairBytes = 128, kMaxWidth = SEQALIGN_BAND_MAX_WIDTH, kHandoffBytes = 8, kBestBytes = 16;   // the walk's eight words (32)
  static constexpr int kMetaWords = 8, kMetaStatus = 1;   // score, status, pos_a, pos_b, end_a, end_b, length, head
  static constexpr const char *kNoWalkText = "";
  static SaBandParams &base(Params &p) { return p.b; }
  static void set_results(Params &p, uint32_t *res, uint64_t n) { p.end_a = res + n; p.end_b = res + 2 * n; }
  static void set_meta(Params &p, uint32_t *meta, uint64_t s0) { p.meta8 = meta + 8 * s0; }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_sw_fill(p, max_width, st); }
  static hipError_t walk(const Params &p, hipStream_t st) { return sa_launch_band_sw_walk(p, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return launch_score_strips(p, l, cols, kAlign, kSw, items, st);
  }
};

struct SwSpanBand {   // seqalign_sw_span_banded(_wide), seqalign_sw_span_band_time_ms (sa_band_span.hip)
  using Params = SaBandSpanParams;
  static constexpr bool kSw = true, kAlign = false;
  static constexpr int kFields = 5;             // score, pos_a, pos_b, len_a, len_b
  static constexpr int kMarkField = 0;
  static constexpr uint64_t kPairBytes = 88, kMaxWidth = SEQALIGN_SPAN_BAND_MAX_WIDTH;
  // a hand-off entry and a best entry as SwStatsBand's: the two payload words are the span's x and y
  static constexpr uint64_t kHandoffBytes = SA_BAND_STATS_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static SaBandParams &base(Params &p) { return p.b; }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
  }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_span(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return sa_launch_band_span_strips({p, l}, cols, items, st);
  }
};

struct SwStatsBand {   // seqalign_sw_stats_banded(_wide), seqalign_sw_stats_band_time_ms (sa_band_stats.hip)
  using Params = SaBandSwStatsParams;
  static constexpr bool kSw = true, kAlign = false;
  static constexpr int kFields = 7;             // the span mode's five, matches, mismatches
  static constexpr int kMarkField = 0;
  static constexpr uint64_t kPairBytes = 96, kMaxWidth = SEQALIGN_SPAN_BAND_MAX_WIDTH;
  // a hand-off entry as NwStatsBand's; the best cell travels with its two words (merge_left_best_span's entry)
  static constexpr uint64_t kHandoffBytes = SA_BAND_STATS_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static SaBandParams &base(Params &p) { return p.b; }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
    p.matches = res + 5 * n; p.mismatches = res + 6 * n;
  }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_sw_stats(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return sa_launch_band_sw_stats_strips({p, l}, cols, items, st);
  }
};

struct SwCountsBand {   // seqalign_sw_counts_banded(_wide), seqalign_sw_counts_band_time_ms (sa_band_counts.hip)
  using Params = SaBandSwCountsParams;
  static constexpr bool kSw = true, kAlign = false;
  static constexpr int kFields = 5;             // score, end_a, end_b, matches, mismatches
  static constexpr int kMarkField = 0;
  // the span mode's bytes and its width rule; no length check: the two payload words are full-word counts
  static constexpr uint64_t kPairBytes = 88, kMaxWidth = SEQALIGN_SPAN_BAND_MAX_WIDTH;
  static constexpr uint64_t kHandoffBytes = SA_BAND_STATS_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static SaBandParams &base(Params &p) { return p.b; }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {   // the span block's arrays by their new names (sa_kernels.h)
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
  }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_sw_counts(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return sa_launch_band_sw_counts_strips({p, l}, cols, items, st);
  }
};

struct SwGapsBand {   // seqalign_sw_gaps_banded(_wide), seqalign_sw_gaps_band_time_ms (sa_band_gaps.hip)
  using Params = SaBandSwGapsParams;
  static constexpr bool kSw = true, kAlign = false;
  static constexpr int kFields = 5;             // score, end_a, end_b, gap_runs_a, gap_runs_b
  static constexpr int kMarkField = 0;
  // the span mode's bytes and its width rule; no length check: the two payload words are full-word run counts
  static constexpr uint64_t kPairBytes = 88, kMaxWidth = SEQALIGN_SPAN_BAND_MAX_WIDTH;
  static constexpr uint64_t kHandoffBytes = SA_BAND_STATS_HANDOFF_BYTES, kBestBytes = SA_SPAN_BEST_BYTES;
  static SaBandParams &base(Params &p) { return p.b; }
  static void set_results(Params &p, uint32_t *res, uint64_t n) {   // the span block's arrays by their new names (sa_kernels.h)
    p.pos_a = res + n; p.pos_b = res + 2 * n; p.len_a = res + 3 * n; p.len_b = res + 4 * n;
  }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_sw_gaps(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return sa_launch_band_sw_gaps_strips({p, l}, cols, items, st);
  }
};

struct NwStatsBand {   // seqalign_nw_stats_banded(_wide), seqalign_nw_stats_band_time_ms (sa_band_nw_stats.hip, sa_band_nw_stats_strips.hip)
  using Params = SaBandNwStatsParams;
  static constexpr bool kSw = false, kAlign = false;
  static constexpr int kFields = 3;             // score, matches, mismatches
  // no alignment inside the band: the end pick's state carries the sticky mark, SA_STATS_NO_WALK in the mismatch word, as in
  // seqalign_nw_stats_batch (StatsTraits::kMarkField).  Not the end value: at large scales a real score lies below INT32_MIN / 2
  static constexpr int kMarkField = 2;
  static constexpr uint64_t kPairBytes = 72, kMaxWidth = SEQALIGN_SPAN_BAND_MAX_WIDTH;
  static constexpr uint64_t kHandoffBytes = SA_BAND_STATS_HANDOFF_BYTES;   // the two values, whose the first is, their payloads
  static constexpr uint64_t kBestBytes = 16;                               // (reserved as in the score modes, not used)
  static SaBandParams &base(Params &p) { return p.b; }
  static void set_results(Params &p, uint32_t *res, uint64_t n) { p.matches = res + n; p.mismatches = res + 2 * n; }
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_nw_stats(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return sa_launch_band_nw_stats_strips({p, l}, cols, items, st);
  }
};

struct NwGapsBand : NwStatsBand {   // seqalign_nw_gaps_banded(_wide), seqalign_nw_gaps_band_time_ms (sa_band_nw_gaps.hip)
  // NwStatsBand with the gap-run kernels: score, gap_runs_a, gap_runs_b; the mark is in the gap_runs_b word (kMarkField = 2)
  static hipError_t launch(const Params &p, uint32_t max_width, hipStream_t st) { return sa_launch_band_nw_gaps(p, max_width, st); }
  static hipError_t launch_strips(const Params &p, const SaBandStripsLayout &l, uint32_t cols, uint64_t items, hipStream_t st) {
    return sa_launch_band_nw_gaps_strips({p, l}, cols, items, st);
  }
};

// a wide launch has (pairs rounded up to 8) x (the chunk's largest strip count) workgroups, most of which return at once when
// one long pair sits among many short ones: a chunk is cut before that product passes this.  One pair alone stays below it
// (len_a < 2^31, 64 columns per strip at least: fewer than 2^25 strips, times 8)
constexpr uint64_t kWideMaxBlocks = (uint64_t)1 << 28;

// ---- band geometry and the checks
struct Band {
  int32_t d_lo;
  uint32_t width;
  uint64_t cells;   // of one matrix in an align mode
};

// the NW calls' bands: band[p] diagonals on either side of the two corner cells' diagonals, clamped to the matrix
struct NwBands {
  const uint32_t *band;
  int operator()(uint64_t p, uint32_t la, uint32_t lb, Band *g, uint64_t *width64) const {
    const int64_t d = (int64_t)la - (int64_t)lb, w = band[p];
    const int64_t d_lo = std::max<int64_t>(-(int64_t)lb, std::min<int64_t>(0, d) - w);
    const int64_t d_hi = std::min<int64_t>((int64_t)la, std::max<int64_t>(0, d) + w);
    *width64 = (uint64_t)(d_hi - d_lo + 1);
    const uint32_t width = (uint32_t)std::min<uint64_t>(*width64, 0xFFFFFFFFu);
    *g = Band{(int32_t)std::max<int64_t>(d_lo, INT32_MIN), width, ((uint64_t)lb + 1) * width};
    return SEQALIGN_OK;
  }
};

// the SW calls': the caller's bounds clipped to [-len_b, len_a].  A band that is empty then is given to the kernels as the one
// diagonal len_a, which has no inner cell: score 0, nothing stored
struct SwBands {
  const int32_t *diag_lo, *diag_hi;
  int operator()(uint64_t p, uint32_t la, uint32_t lb, Band *g, uint64_t *width64) const {
    if (diag_lo[p] > diag_hi[p]) {
      set_last_error("pair " + std::to_string(p) + ": diag_lo " + std::to_string(diag_lo[p]) + " is above diag_hi " + std::to_string(diag_hi[p]));
      return SEQALIGN_E_ARG;
    }
    const int64_t d_lo = std::max<int64_t>(diag_lo[p], -(int64_t)lb), d_hi = std::min<int64_t>(diag_hi[p], (int64_t)la);
    if (d_lo > d_hi) { *width64 = 0; *g = Band{(int32_t)la, 1, 0}; return SEQALIGN_OK; }
    *width64 = (uint64_t)(d_hi - d_lo + 1);
    int64_t j0, j1;
    sa_band_sw_rows(la, lb, d_lo, d_hi, &j0, &j1);
    *g = Band{(int32_t)d_lo, (uint32_t)std::min<uint64_t>(*width64, 0xFFFFFFFFu), j1 < j0 ? 0 : (uint64_t)(j1 - j0 + 1) * *width64};
    return SEQALIGN_OK;
  }
};

// argument checks and band geometry of mode M, before any device work.  Per pair, in this order: what `bands` refuses, the
// lengths, and (not in a wide call) the width against the mode's cap
template <class M, class Bands>
int check_band_batch(const seqalign_batch_t *b, const Bands &bands, std::vector<Band> &geom, bool wide = false) {
  if (!batch_readable(b)) return SEQALIGN_E_ARG;
  geom.resize(b->n_pairs);
  for (uint64_t p = 0; p < b->n_pairs; ++p) {
    const uint32_t la = b->len_a[p], lb = b->len_b[p];
    uint64_t width = 0;
    const int rc = bands(p, la, lb, &geom[p], &width);
    if (rc) return rc;
    if ((uint64_t)la + lb >= ((uint64_t)1 << 31)) {
      set_last_error("pair " + std::to_string(p) + ": len_a + len_b is 2^31 or more");
      return SEQALIGN_E_TOO_LARGE;
    }
    if (!wide && width > M::kMaxWidth) {
      set_last_error("pair " + std::to_string(p) + ": a band of " + std::to_string(width) + " diagonals, at most " +
                     std::to_string(M::kMaxWidth) + " are supported");
      return SEQALIGN_E_TOO_LARGE;
    }
  }
  return SEQALIGN_OK;
}

// the SW statistics calls' checks in the header's order: the band (a wide call: without the width), then sw_stats' length limit
int check_sw_stats_band_batch(const seqalign_batch_t *batch, const int32_t *diag_lo, const int32_t *diag_hi, std::vector<Band> &geom,
                              bool wide = false) {
  const int rc = check_band_batch<SwStatsBand>(batch, SwBands{diag_lo, diag_hi}, geom, wide);
  return rc ? rc : sw_stats_check_batch(batch);
}

// ---- the wide calls: a pair's strips of `cols` columns, and what they add to its bytes -- per strip a hand-off column of
// `width` entries of the mode's bytes (8; the statistics: 32), a progress word (4) and a best-cell entry of the mode's bytes (16;
// SW statistics: 32), and per pair two more descriptors (16) and a front word (4)
uint64_t wide_strips(uint32_t la, uint32_t cols) { return la ? ((uint64_t)la + cols - 1) / cols : 1; }
uint64_t wide_bytes(uint32_t la, uint32_t width, uint32_t cols, uint64_t entry_bytes, uint64_t best_bytes) {
  return wide_strips(la, cols) * (entry_bytes * (uint64_t)width + 4 + best_bytes) + 20;
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

// a pair's device bytes in mode M: the sequences (an align mode: the strings besides, and the band's cells), the mode's fixed
// bytes, the strips' scratch of a wide call
template <class M>
uint64_t pair_bytes(uint32_t la, uint32_t lb, const Band &g, uint32_t wide_cols) {
  const uint64_t seq = (uint64_t)la + lb;
  return (wide_cols ? wide_bytes(la, g.width, wide_cols, M::kHandoffBytes, M::kBestBytes) : 0) + (M::kAlign ? 12 * g.cells + 3 * seq : seq) + M::kPairBytes;
}

// ---- One chunk of a call in mode M laid out and uploaded; launch() enqueues its kernels on ctx->stream
template <class M>
struct BandChunkRun {
  using Params = typename M::Params;
  seqalign_ctx *ctx = nullptr;
  const seqalign_dev_scoring *sc = nullptr;
  // classes by band width; the descriptors behind the shared ones: mat_off, str_off (wide: slot_off, hand_off), width, d_lo
  ChunkStage<SA_SCORE_ROW_CLASSES> stage;
  uint64_t n = 0, seq_bytes = 0;
  uint32_t *d_res = nullptr;   // [4] header (err_flag; wide: give-up word), then M::kFields arrays of n words: M::set_results
  uint64_t cells = 0;
  // the wide calls: columns per strip (0: the narrow calls), one launch per chunk over all its slots
  uint32_t wide = 0, strips_per_pair = 0;
  uint64_t slots = 0, hand_total = 0, busy_strips = 0;

  BandChunkRun(seqalign_ctx *c, const seqalign_dev_scoring *scoring, uint32_t wide_cols) : ctx(c), sc(scoring), wide(wide_cols) { stage.ctx = c; }

  // slot -> where its strings start in the chunk's string buffers: where its sequences do (a pair's strings are len_a + len_b
  // bytes at most); read from the pinned descriptors, which stay as laid out until the next chunk
  uint64_t str_at(uint64_t s) const { return stage.h_off_a[s]; }
  size_t result_words() const { return 4 + M::kFields * n; }

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
    if (rc || (rc = ctx->best_score.reserve(4 * result_words()))) return rc;
    if constexpr (M::kAlign)
      if ((rc = ctx->long_block.reserve(12 * cells + 64)) || (rc = ctx->t_out_a.reserve(seq_bytes + 16)) ||
          (rc = ctx->t_out_b.reserve(seq_bytes + 16)) || (rc = ctx->t_meta.reserve(4 * M::kMetaWords * n)))
        return rc;
    // wide: progress words, the ticket counter and the pairs' front words behind them, then (16-byte aligned) the best-cell
    // entries; the hand-off columns
    if (wide && ((rc = ctx->strip_progress.reserve(4 * (slots + n + 8) + M::kBestBytes * slots + 16)) || (rc = ctx->score_handoff.reserve(M::kHandoffBytes * hand_total + 16))))
      return rc;
    d_res = ctx->best_score.as<uint32_t>();
    return stage.upload();
  }

  // the kernels' block for slots [s0, s0 + m)
  Params params(uint64_t s0, uint64_t m) const {
    Params p{};
    SaBandParams &b = M::base(p);
    b.f = score_fill_params(sc);
    stage.set_slots(b.f, s0, m);
    b.f.mat_off = stage.d_u64(0) + s0;
    b.d_lo = stage.d_u32<int32_t>(1) + s0; b.width = stage.d_u32(0) + s0;
    b.score = reinterpret_cast<int32_t *>(d_res + 4) + s0;
    b.err_flag = d_res;
    M::set_results(p, d_res + 4 + s0, n);
    if constexpr (M::kAlign) {
      b.f.M = ctx->long_block.as<int32_t>(); b.f.A = b.f.M + cells; b.f.B = b.f.A + cells;
      b.str_off = stage.d_u64(1) + s0;
      b.out_a = ctx->t_out_a.as<char>(); b.out_b = ctx->t_out_b.as<char>();
      M::set_meta(p, ctx->t_meta.as<uint32_t>(), s0);
    }
    return p;
  }

  // the wide calls: one launch over all slots of the chunk, strips_per_pair the chunk's maximum
  int launch_wide() {
    hipStream_t st = ctx->stream;
    SaBandStripsLayout w{};
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
    const hipError_t e = M::launch_strips(params(0, n), w, wide, busy_strips, st);
    if (e != hipSuccess) return fail_hip(e, "band strips kernel launch");
    return SEQALIGN_OK;
  }

  // wide: the give-up word of the header brought home in h: slot + 1 of the first pair one of whose strips gave up
  int fail_if_gave_up(const uint32_t *h) {
    if (!wide || !h[1]) return SEQALIGN_OK;
    const uint64_t slot = h[1] - 1;
    set_last_error("pair " + std::to_string(stage.first + (slot < n ? stage.order[slot] : 0)) + ": band strip hand-off timed out");
    return SEQALIGN_E_HIP;
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
      const hipError_t e = M::launch(params(s0, m), stage.cls_max[x], st);
      if (e != hipSuccess) return fail_hip(e, "band kernel launch");
    }
    if constexpr (M::kAlign) {
      const hipError_t e = M::walk(params(0, n), st);
      if (e != hipSuccess) return fail_hip(e, "band walk launch");
    }
    return SEQALIGN_OK;
  }

  // the score family's way home: the header and M::kFields arrays of n words, array 0 to out_score, array f to out[f - 1].  The
  // lowest pair of the chunk whose sweep met a band cell without a score is named; kMarkField: so is the lowest whose end
  // pick carries the mark, SEQALIGN_E_TRACEBACK, and between the two the lower pair's code is the call's, as in
  // seqalign_nw_stats_batch
  int finish_words(int32_t *out_score, uint32_t *const *out) {
    int rc;
    if ((rc = ctx->h_misc.reserve(4 * result_words()))) return rc;
    uint32_t *h = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h, d_res, 4 * result_words(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    if ((rc = fail_if_gave_up(h))) return rc;
    uint64_t unknown = ~0ull;   // the chunk's lowest pair without a score, as a batch index
    if (h[0]) rc = stage.fail_from_status(&unknown);
    if constexpr (M::kMarkField > 0)
      if (!rc || rc == SEQALIGN_E_UNKNOWN_PAIR) {
        uint64_t no_walk = ~0ull;
        const uint32_t *w = h + 4 + (uint64_t)M::kMarkField * n;
        for (uint64_t s = 0; s < n; ++s)
          if (w[s] & SA_STATS_NO_WALK) no_walk = std::min<uint64_t>(no_walk, stage.first + stage.order[s]);
        if (no_walk < unknown) {
          set_last_error("pair " + std::to_string(no_walk) + ": traceback failed (no alignment inside the band)");
          return SEQALIGN_E_TRACEBACK;
        }
      }
    if (rc) return rc;
    stage.scatter(h + 4, M::kFields, out_score, out);
    return SEQALIGN_OK;
  }

  // the align modes' way home up to the delivery: the walk's records (ctx->h_tmeta) and the strings (ctx->h_ta, ctx->h_tb) in
  // slot order, and with them the wide calls' give-up word; the lowest pair whose walk left a status is the call's error
  int fetch_walks() {
    int rc;
    const size_t meta_bytes = 4 * M::kMetaWords * n;
    if ((rc = ctx->h_tmeta.reserve(meta_bytes)) || (rc = ctx->h_ta.reserve(seq_bytes + 16)) || (rc = ctx->h_tb.reserve(seq_bytes + 16))) return rc;
    hipStream_t st = ctx->stream;
    if (wide) {
      if ((rc = ctx->h_misc.reserve(16))) return rc;
      HIP_TRY(hipMemcpyAsync(ctx->h_misc.p, d_res, 16, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(ctx->h_tmeta.p, ctx->t_meta.p, meta_bytes, hipMemcpyDeviceToHost, st));
    if (seq_bytes) {
      HIP_TRY(hipMemcpyAsync(ctx->h_ta.p, ctx->t_out_a.p, seq_bytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(ctx->h_tb.p, ctx->t_out_b.p, seq_bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(stream_wait_spinning(st));
    if (wide && (rc = fail_if_gave_up(ctx->h_misc.as<uint32_t>()))) return rc;
    const uint32_t *status = ctx->h_tmeta.as<uint32_t>() + M::kMetaStatus;
    uint64_t worst = ~0ull;
    uint32_t worst_code = 0;
    for (uint64_t s = 0; s < n; ++s)
      if (status[M::kMetaWords * s] && stage.order[s] < worst) { worst = stage.order[s]; worst_code = status[M::kMetaWords * s]; }
    if (worst == ~0ull) return SEQALIGN_OK;
    if (worst_code == SEQALIGN_E_UNKNOWN_PAIR) return fail_unknown_pair(stage.first + worst);
    set_last_error("pair " + std::to_string(stage.first + worst) + ": traceback failed" + M::kNoWalkText);
    return (int)worst_code;
  }

  // banded SW: the chunk's hits in pair order, under seqalign_sw_align_long's capacity rule.  A pair's own error comes before
  // SEQALIGN_E_NOMEM and nothing of the chunk is delivered then.
  int finish_sw_align(const int32_t *min_score, HitSink &sink, uint64_t *n_hits) {
    const int rc = fetch_walks();
    if (rc) return rc;
    const uint64_t first = stage.first;
    const uint32_t *meta = ctx->h_tmeta.as<uint32_t>();
    std::vector<uint32_t> slot_of(n);
    for (uint64_t s = 0; s < n; ++s) slot_of[stage.order[s]] = (uint32_t)s;
    const char *ha = ctx->h_ta.as<char>(), *hb = ctx->h_tb.as<char>();
    for (uint64_t k = 0; k < n; ++k) {
      const uint64_t s = slot_of[k], p = first + k;
      const uint32_t *m = meta + 8 * s;
      const int32_t score = (int32_t)m[0];
      if (score <= 0 || score < min_score[p]) continue;   // no hit
      const uint32_t len = m[6], head = m[7];
      const seqalign_sw_hit_t h{p, score, m[2], m[3], m[4] - m[2], m[5] - m[3], len, 0};   // smith_waterman.c:251-255
      if (!sink.put(ctx, h, ha + str_at(s) + head, hb + str_at(s) + head)) return SEQALIGN_E_NOMEM;
      *n_hits = sink.found;
    }
    return SEQALIGN_OK;
  }

  // banded NW: every pair's strings to the caller's offsets
  int finish_align(const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score) {
    const int rc = fetch_walks();
    if (rc) return rc;
    const uint64_t first = stage.first;
    const std::vector<uint32_t> &order = stage.order;
    const uint32_t *meta = ctx->h_tmeta.as<uint32_t>();
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

// ---- what every call does behind its checks: the device, the scoring, the batch admitted, the chunks planned -- cut_chunks
// with mode M's bytes per pair, the band cells summed per chunk and a wide launch's grid capped
template <class M>
struct BandPlan {
  seqalign_dev_scoring *sc = nullptr;
  uint32_t cols = 0;   // of a wide call's strips
  std::vector<ByteChunk> chunks;

  int make(seqalign_ctx_t *ctx, const seqalign_batch_t *b, const scoring_t *scoring, const std::vector<Band> &geom, bool wide) {
    int rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((rc = cached_scoring(ctx, scoring, M::kSw ? 1 : 0, &sc))) return rc;
    if ((rc = admit_batch(sc, b, SA_FRAMES_BAND))) return rc;
    cols = wide ? wide_strip_cols(ctx, b->n_pairs) : 0;
    return cut_chunks(b, ctx->chunk_budget, [&](uint64_t p) {
      const uint32_t la = b->len_a[p];
      return PairNeed{pair_bytes<M>(la, b->len_b[p], geom[p], cols), geom[p].cells, cols ? wide_strips(la, cols) : 0};
    }, chunks, true, kWideMaxBlocks);
  }
};

// A banded call behind its checks: every chunk prepared, launched and brought home by finish(run)
template <class M, class Finish>
int band_call(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const std::vector<Band> &geom, bool wide, Finish finish) {
  int rc;
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  BandPlan<M> plan;
  if ((rc = plan.make(ctx, batch, scoring, geom, wide))) return rc;
  StreamSyncOnExit sync(ctx->stream);
  for (const ByteChunk &c : plan.chunks) {
    BandChunkRun<M> run(ctx, plan.sc, plan.cols);
    if ((rc = run.prepare(batch, geom, c)) || (rc = run.launch()) || (rc = finish(run))) return rc;
  }
  return SEQALIGN_OK;
}

// mode M's launches of one chunk, `repeats` times between HIP events
template <class M>
int band_time(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const std::vector<Band> &geom, int repeats,
              float *ms_each, const char *name) {
  int rc;
  if (batch->n_pairs == 0) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  BandPlan<M> plan;
  if ((rc = plan.make(ctx, batch, scoring, geom, false))) return rc;
  if (plan.chunks.size() != 1) { set_last_error(std::string(name) + ": the batch does not fit one chunk"); return SEQALIGN_E_ARG; }
  StreamSyncOnExit sync(ctx->stream);
  BandChunkRun<M> run(ctx, plan.sc, 0);
  if ((rc = run.prepare(batch, geom, plan.chunks[0]))) return rc;
  return time_launches(ctx->stream, repeats, ms_each, [&] { return run.launch(); });
}

// ---- the contracts, each the body of its narrow call and of its wide one (any width; kernel:
// sa_band_strips.hip)
int nw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const uint32_t *band, int32_t *out_score,
                    bool wide) {
  if (!ctx || !batch || !scoring || !band || !out_score) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<NwScoreBand>(batch, NwBands{band}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  return band_call<NwScoreBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, nullptr); });
}

int nw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const uint32_t *band, const uint64_t *str_off,
                    char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score, bool wide) {
  if (!ctx || !batch || !scoring || !band || !str_off || !out_a || !out_b || !out_len || !out_score) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<NwAlignBand>(batch, NwBands{band}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  return band_call<NwAlignBand>(ctx, batch, scoring, geom, wide,
                                [&](auto &run) { return run.finish_align(str_off, out_a, out_b, out_len, out_score); });
}

int sw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo, const int32_t *diag_hi,
                    int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_end_a || !out_end_b) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwScoreBand>(batch, SwBands{diag_lo, diag_hi}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[2] = {out_end_a, out_end_b};
  return band_call<SwScoreBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, out); });
}

int sw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo, const int32_t *diag_hi,
                    const int32_t *min_score, seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b,
                    uint64_t str_cap, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !min_score || !hits || !n_hits || !out_a || !out_b) return SEQALIGN_E_ARG;
  *n_hits = 0;
  std::vector<Band> geom;
  int rc = check_band_batch<SwAlignBand>(batch, SwBands{diag_lo, diag_hi}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  HitSink sink{hits, hit_cap, out_a, out_b, str_cap};
  return band_call<SwAlignBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_sw_align(min_score, sink, n_hits); });
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
  int rc = check_band_batch<NwScoreBand>(batch, NwBands{band}, geom);
  if (rc) return rc;
  return band_time<NwScoreBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_band_score_time_ms");
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

extern "C" int seqalign_sw_band_score_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwScoreBand>(batch, SwBands{diag_lo, diag_hi}, geom);
  if (rc) return rc;
  return band_time<SwScoreBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_sw_band_score_time_ms");
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

// banded SW hit spans: the narrow call, and the wide form without the width check (kernel: band_payload_strips_kernel, sa_band_frame.hpp, by sa_band_span.hip)
static int sw_span_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo,
                          const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a,
                          uint32_t *out_len_b, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwSpanBand>(batch, SwBands{diag_lo, diag_hi}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[4] = {out_pos_a, out_pos_b, out_len_a, out_len_b};
  return band_call<SwSpanBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, out); });
}

extern "C" int seqalign_sw_span_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a,
                                       uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b) {
  return sw_span_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_pos_a, out_pos_b, out_len_a, out_len_b, false);
}

extern "C" int seqalign_sw_span_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                            const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a,
                                            uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b) {
  return sw_span_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_pos_a, out_pos_b, out_len_a, out_len_b, true);
}

extern "C" int seqalign_sw_span_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwSpanBand>(batch, SwBands{diag_lo, diag_hi}, geom);
  if (rc) return rc;
  return band_time<SwSpanBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_sw_span_band_time_ms");
}

// banded SW statistics: the two passes of checks in the header's order; the wide form: without the width check (kernel:
// band_payload_strips_kernel, sa_band_frame.hpp, by sa_band_stats.hip)
static int sw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo,
                           const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a,
                           uint32_t *out_len_b, uint32_t *out_matches, uint32_t *out_mismatches, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b ||
      !out_matches || !out_mismatches)
    return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_stats_band_batch(batch, diag_lo, diag_hi, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[6] = {out_pos_a, out_pos_b, out_len_a, out_len_b, out_matches, out_mismatches};
  return band_call<SwStatsBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, out); });
}

extern "C" int seqalign_sw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a,
                                        uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b, uint32_t *out_matches,
                                        uint32_t *out_mismatches) {
  return sw_stats_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_pos_a, out_pos_b, out_len_a, out_len_b, out_matches,
                         out_mismatches, false);
}

extern "C" int seqalign_sw_stats_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_pos_a,
                                             uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b, uint32_t *out_matches,
                                             uint32_t *out_mismatches) {
  return sw_stats_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_pos_a, out_pos_b, out_len_a, out_len_b, out_matches,
                         out_mismatches, true);
}

extern "C" int seqalign_sw_stats_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_sw_stats_band_batch(batch, diag_lo, diag_hi, geom);
  if (rc) return rc;
  return band_time<SwStatsBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_sw_stats_band_time_ms");
}

// banded SW identity counts at any length: seqalign_sw_span_banded's checks in its order and nothing else; the wide form:
// without the width check (kernels: sa_band_frame.hpp's two shells, by sa_band_counts.hip)
static int sw_counts_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo,
                            const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b,
                            uint32_t *out_matches, uint32_t *out_mismatches, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_end_a || !out_end_b || !out_matches || !out_mismatches) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwCountsBand>(batch, SwBands{diag_lo, diag_hi}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[4] = {out_end_a, out_end_b, out_matches, out_mismatches};
  return band_call<SwCountsBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, out); });
}

extern "C" int seqalign_sw_counts_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                         const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                                         uint32_t *out_end_b, uint32_t *out_matches, uint32_t *out_mismatches) {
  return sw_counts_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_end_a, out_end_b, out_matches, out_mismatches, false);
}

extern "C" int seqalign_sw_counts_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score,
                                              uint32_t *out_end_a, uint32_t *out_end_b, uint32_t *out_matches,
                                              uint32_t *out_mismatches) {
  return sw_counts_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_end_a, out_end_b, out_matches, out_mismatches, true);
}

extern "C" int seqalign_sw_counts_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                               const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwCountsBand>(batch, SwBands{diag_lo, diag_hi}, geom);
  if (rc) return rc;
  return band_time<SwCountsBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_sw_counts_band_time_ms");
}

// banded SW gap-run counts at any length: seqalign_sw_span_banded's checks in its order and nothing else; the wide form:
// without the width check (kernels: sa_band_frame.hpp's two shells, by sa_band_gaps.hip)
static int sw_gaps_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const int32_t *diag_lo,
                            const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b,
                            uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b, bool wide) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || !out_score || !out_end_a || !out_end_b || !out_gap_runs_a || !out_gap_runs_b) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwGapsBand>(batch, SwBands{diag_lo, diag_hi}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[4] = {out_end_a, out_end_b, out_gap_runs_a, out_gap_runs_b};
  return band_call<SwGapsBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, out); });
}

extern "C" int seqalign_sw_gaps_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                         const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                                         uint32_t *out_end_b, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b) {
  return sw_gaps_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_end_a, out_end_b, out_gap_runs_a, out_gap_runs_b, false);
}

extern "C" int seqalign_sw_gaps_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score,
                                              uint32_t *out_end_a, uint32_t *out_end_b, uint32_t *out_gap_runs_a,
                                              uint32_t *out_gap_runs_b) {
  return sw_gaps_banded(ctx, batch, scoring, diag_lo, diag_hi, out_score, out_end_a, out_end_b, out_gap_runs_a, out_gap_runs_b, true);
}

extern "C" int seqalign_sw_gaps_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                               const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !diag_lo || !diag_hi || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<SwGapsBand>(batch, SwBands{diag_lo, diag_hi}, geom);
  if (rc) return rc;
  return band_time<SwGapsBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_sw_gaps_band_time_ms");
}

// banded NW statistics: seqalign_nw_score_banded's checks in its order, with the span cap on the width; the wide form: without
// it (kernel: sa_band_nw_stats_strips.hip)
static int nw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const uint32_t *band,
                           int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches, bool wide) {
  if (!ctx || !batch || !scoring || !band || !out_score || !out_matches || !out_mismatches) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<NwStatsBand>(batch, NwBands{band}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[2] = {out_matches, out_mismatches};
  return band_call<NwStatsBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, out); });
}

extern "C" int seqalign_nw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                        const uint32_t *band, int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches) {
  return nw_stats_banded(ctx, batch, scoring, band, out_score, out_matches, out_mismatches, false);
}

extern "C" int seqalign_nw_stats_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const uint32_t *band, int32_t *out_score, uint32_t *out_matches,
                                             uint32_t *out_mismatches) {
  return nw_stats_banded(ctx, batch, scoring, band, out_score, out_matches, out_mismatches, true);
}

extern "C" int seqalign_nw_stats_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                              const uint32_t *band, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !band || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<NwStatsBand>(batch, NwBands{band}, geom);
  if (rc) return rc;
  return band_time<NwStatsBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_nw_stats_band_time_ms");
}

// banded NW gap-run counts: seqalign_nw_stats_banded[_wide]'s checks in their order (kernels: sa_band_nw_gaps.hip)
static int nw_gaps_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, const uint32_t *band,
                          int32_t *out_score, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b, bool wide) {
  if (!ctx || !batch || !scoring || !band || !out_score || !out_gap_runs_a || !out_gap_runs_b) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<NwGapsBand>(batch, NwBands{band}, geom, wide);
  if (rc) return rc;
  CallScope scope(ctx);
  uint32_t *const out[2] = {out_gap_runs_a, out_gap_runs_b};
  return band_call<NwGapsBand>(ctx, batch, scoring, geom, wide, [&](auto &run) { return run.finish_words(out_score, out); });
}

extern "C" int seqalign_nw_gaps_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       const uint32_t *band, int32_t *out_score, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b) {
  return nw_gaps_banded(ctx, batch, scoring, band, out_score, out_gap_runs_a, out_gap_runs_b, false);
}

extern "C" int seqalign_nw_gaps_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                            const uint32_t *band, int32_t *out_score, uint32_t *out_gap_runs_a,
                                            uint32_t *out_gap_runs_b) {
  return nw_gaps_banded(ctx, batch, scoring, band, out_score, out_gap_runs_a, out_gap_runs_b, true);
}

extern "C" int seqalign_nw_gaps_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                             const uint32_t *band, int repeats, float *ms_each) {
  if (!ctx || !batch || !scoring || !band || repeats <= 0 || !ms_each) return SEQALIGN_E_ARG;
  std::vector<Band> geom;
  int rc = check_band_batch<NwGapsBand>(batch, NwBands{band}, geom);
  if (rc) return rc;
  return band_time<NwGapsBand>(ctx, batch, scoring, geom, repeats, ms_each, "seqalign_nw_gaps_band_time_ms");
}
