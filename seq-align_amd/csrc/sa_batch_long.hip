// sa_batch_long.hip -- seqalign_nw_align_long / seqalign_sw_align_long: the alignments of seqalign_nw_batch and
// seqalign_sw_batch(max_hits = 1), bytes for bytes, for pairs of any size (the kernels: sa_align_long.hip).
//
// Pairs run one after another.  Per pair: the sequences go up; the forward pass stores the checkpoint rows (and finds the SW
// best cell); then, from where the walk stands, block after block: fill rows [y0, y] x columns [0, x], walk them, bring the
// walk's 64-byte state home to learn the next block.  The strings come home once, at the end.
//
// Device memory of a pair, with R rows per block, C = len_a + 1:
//   12 C floor((len_b - 1) / R)  checkpoints      12 C (min(R, len_b) + 1)  the block
//   8 (ceil(len_a / 512) - 1) (len_b + 1)  the forward pass's hand-off columns      3 (len_a + len_b)  sequences and strings
// R: the option long_block_rows, or (0) the largest that keeps the block under 2^31 cells and the whole within the
// context's chunk budget -- few blocks: each one costs the strip pipeline's fill, 64 rows per strip, besides its rows.
#include <cmath>

#include "sa_ctx.hpp"

using namespace sa_host;

namespace {

constexpr uint64_t kBlockCellsMax = ((uint64_t)1 << 31) - 1;   // in-block offsets stay 32-bit, as in the existing walkers

uint32_t long_strips(uint32_t cols) { return cols ? (uint32_t)(((uint64_t)cols + SA_LONG_STRIP_COLS - 1) / SA_LONG_STRIP_COLS) : 1u; }

struct LongPlan {
  uint32_t R = 1;          // rows per block (>= 1)
  uint64_t nck = 0;        // checkpoint rows
  uint64_t block_rows = 1; // rows of the largest block
  uint64_t need = 0;       // device bytes
};

LongPlan long_plan(uint32_t la, uint32_t lb, uint64_t R) {
  LongPlan pl;
  pl.R = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(R, 0xFFFFFFFFull));
  pl.nck = lb ? (lb - 1ull) / pl.R : 0;
  pl.block_rows = std::min<uint64_t>(pl.R, lb) + 1;
  const uint64_t C = (uint64_t)la + 1, strips = long_strips(la);
  pl.need = 12 * C * pl.nck + 12 * C * pl.block_rows + 8 * (strips - 1) * ((uint64_t)lb + 1) + 3 * ((uint64_t)la + lb) +
            20 * strips + 4096;
  return pl;
}

// rows per block for one pair: forced (option long_block_rows), or the largest that fits; 0 with a message: E_NOMEM
int choose_plan(const seqalign_ctx *ctx, uint64_t pair, uint32_t la, uint32_t lb, LongPlan &out) {
  const uint64_t budget = ctx->chunk_budget, C = (uint64_t)la + 1;
  const uint64_t r_cells = kBlockCellsMax / C;   // block rows (R + 1) * C <= 2^31 - 1
  if (r_cells < 2) {
    set_last_error("pair " + std::to_string(pair) + ": a row of " + std::to_string(C) + " cells leaves no block of two rows under 2^31 cells");
    return SEQALIGN_E_NOMEM;
  }
  const uint64_t r_max = r_cells - 1;
  LongPlan pl;
  if (ctx->opt.long_block_rows) {
    pl = long_plan(la, lb, std::min<uint64_t>(ctx->opt.long_block_rows, r_max));
  } else {
    const uint64_t hi = std::max<uint64_t>(1, std::min<uint64_t>(lb, r_max));
    pl = long_plan(la, lb, hi);
    if (pl.need > budget) {
      // need(R) is convex with its minimum near sqrt(len_b): the largest R in [that, hi] that fits
      uint64_t lo = std::min<uint64_t>(hi, std::max<uint64_t>(1, (uint64_t)std::sqrt((double)lb)));
      pl = long_plan(la, lb, lo);
      if (pl.need <= budget) {
        uint64_t a = lo, b = hi;   // need(a) fits, need(b) does not
        while (b - a > 1) {
          const uint64_t m = a + (b - a) / 2;
          if (long_plan(la, lb, m).need <= budget) a = m; else b = m;
        }
        pl = long_plan(la, lb, a);
      }
    }
  }
  if (pl.need > budget) {
    set_last_error("pair " + std::to_string(pair) + ": " + std::to_string(pl.need) + " bytes of device memory needed (checkpoints and a block of " +
                   std::to_string(pl.R) + " rows), the chunk budget is " + std::to_string(budget));
    return SEQALIGN_E_NOMEM;
  }
  out = pl;
  return SEQALIGN_OK;
}

// argument checks, before any device work
int check_long_batch(const seqalign_batch_t *b) {
  if (!batch_readable(b)) return SEQALIGN_E_ARG;
  for (uint64_t p = 0; p < b->n_pairs; ++p)
    if ((uint64_t)b->len_a[p] + b->len_b[p] >= 0xFFFFFFFFull) return SEQALIGN_E_TOO_LARGE;
  return SEQALIGN_OK;
}

struct LongMeta {        // what comes home after each walk (pinned)
  SaLongWalk walk;
  int32_t result[4];     // forward: score, end_a, end_b, err_flag
  uint64_t status;       // the lowest cell without a score (~0: none)
  uint64_t pad;
};
static_assert(sizeof(LongMeta) % 16 == 0, "LongMeta");

// One pair, start to end.  On SEQALIGN_OK *has_alignment says whether there is an alignment (SW: a hit of score > 0 and
// >= min_score); its strings are in the pinned h_ta (a) / h_tb (b), `len` long, with the walk's end state in *meta.
struct LongPair {
  seqalign_ctx *ctx;
  const seqalign_dev_scoring *sc;
  bool is_sw;

  int run(const seqalign_batch_t *b, uint64_t pair, int32_t min_score, bool *has_alignment, uint32_t *len, LongMeta *meta) {
    int rc;
    *has_alignment = false;
    const uint32_t la = b->len_a[pair], lb = b->len_b[pair];
    LongPlan pl;
    if ((rc = choose_plan(ctx, pair, la, lb, pl))) return rc;
    const uint64_t C = (uint64_t)la + 1, seq = (uint64_t)la + lb;
    const uint32_t strips_fwd = long_strips(la);
    hipStream_t st = ctx->stream;

    // sequences + descriptors (off_a, off_b: u64; len_a, len_b: u32) up
    if ((rc = ctx->h_arena.reserve(seq + 16)) || (rc = ctx->h_desc.reserve(64)) || (rc = ctx->h_tmeta.reserve(sizeof(LongMeta))) ||
        (rc = ctx->arena.reserve(seq + 16)) || (rc = ctx->off_a.reserve(64)) || (rc = ctx->t_meta.reserve(sizeof(LongMeta))) ||
        (rc = ctx->strip_progress.reserve(sa_strip_progress_bytes(strips_fwd))) ||
        (rc = ctx->t_out_a.reserve(seq + 16)) || (rc = ctx->t_out_b.reserve(seq + 16)) ||
        (rc = ctx->long_ckpt.reserve(12 * C * pl.nck + 16)) || (rc = ctx->long_block.reserve(12 * C * pl.block_rows + 16)))
      return rc;
    if (strips_fwd > 1 && (rc = ctx->score_handoff.reserve(8 * (uint64_t)(strips_fwd - 1) * ((uint64_t)lb + 1) + 16))) return rc;
    StreamSyncOnExit sync(st);
    uint8_t *h_seq = ctx->h_arena.as<uint8_t>();
    parallel_memcpy(h_seq, b->arena + b->off_a[pair], la);
    parallel_memcpy(h_seq + la, b->arena + b->off_b[pair], lb);
    uint64_t *h_d = ctx->h_desc.as<uint64_t>();
    h_d[0] = 0; h_d[1] = la;
    reinterpret_cast<uint32_t *>(h_d + 2)[0] = la; reinterpret_cast<uint32_t *>(h_d + 2)[1] = lb;
    if (seq) HIP_TRY(hipMemcpyAsync(ctx->arena.p, h_seq, seq, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ctx->off_a.p, h_d, 24, hipMemcpyHostToDevice, st));
    LongMeta *h_meta = ctx->h_tmeta.as<LongMeta>();
    memset(h_meta, 0, sizeof(LongMeta));
    h_meta->status = ~0ull;
    h_meta->walk.head = la + lb;
    h_meta->walk.x = la; h_meta->walk.y = lb;   // (NW: the end cell; SW: set below, from the forward pass)
    HIP_TRY(hipMemcpyAsync(ctx->t_meta.p, h_meta, sizeof(LongMeta), hipMemcpyHostToDevice, st));
    LongMeta *d_meta = ctx->t_meta.as<LongMeta>();

    SaLongParams p;
    memset(&p, 0, sizeof(p));
    p.f = score_fill_params(sc);
    p.f.arena = ctx->arena.as<uint8_t>();
    p.f.off_a = ctx->off_a.as<uint64_t>(); p.f.off_b = p.f.off_a + 1;
    p.f.len_a = reinterpret_cast<const uint32_t *>(p.f.off_a + 2); p.f.len_b = p.f.len_a + 1;
    p.f.status = &d_meta->status;
    p.f.n_pairs = 1;
    p.R = pl.R;
    p.ckpt = ctx->long_ckpt.as<int32_t>();
    p.progress = ctx->strip_progress.as<uint32_t>();
    p.walk = &d_meta->walk;
    p.out_a = ctx->t_out_a.as<char>(); p.out_b = ctx->t_out_b.as<char>();

    // forward: the checkpoints, and the SW best cell (NW without checkpoints: the one block covers the whole matrix and
    // reports a cell without a score itself)
    uint32_t x = la, y = lb;
    if (is_sw || pl.nck) {
      p.strips = strips_fwd;
      p.handoff = strips_fwd > 1 ? ctx->score_handoff.as<int32_t>() : nullptr;
      p.strip_best = p.progress + sa_strip_best_word(strips_fwd);
      p.result = d_meta->result;
      HIP_TRY(hipMemsetAsync(p.progress, 0, 4 * (strips_fwd + 1), st));
      hipError_t e = sa_launch_long_forward(p, is_sw, st);
      if (e != hipSuccess) return fail_hip(e, "long forward launch");
      HIP_TRY(hipMemcpyAsync(h_meta, d_meta, sizeof(LongMeta), hipMemcpyDeviceToHost, st));
      HIP_TRY(stream_wait_spinning(st));
      if (h_meta->result[3] || h_meta->status != ~0ull) return fail_unknown_pair(pair);
      if (is_sw) {
        const int32_t best = h_meta->result[0];
        if (best <= 0 || best < min_score) return SEQALIGN_OK;   // no hit
        x = (uint32_t)h_meta->result[1]; y = (uint32_t)h_meta->result[2];
      }
    } else if (is_sw) {
      return SEQALIGN_OK;
    }

    // block after block
    if (is_sw) {
      h_meta->walk.x = x; h_meta->walk.y = y;
      HIP_TRY(hipMemcpyAsync(&d_meta->walk, &h_meta->walk, sizeof(SaLongWalk), hipMemcpyHostToDevice, st));
    }
    const uint64_t slot = C * pl.block_rows;   // one matrix of the largest block
    p.f.M = ctx->long_block.as<int32_t>(); p.f.A = p.f.M + slot; p.f.B = p.f.A + slot;
    for (bool first = true;; first = false) {
      const uint32_t y0 = (y == 0 || pl.nck == 0) ? 0u : ((y - 1) / pl.R) * pl.R;
      p.y0 = y0; p.y1 = y; p.x = x;
      p.strips = long_strips(x);
      HIP_TRY(hipMemsetAsync(p.progress, 0, 4 * (p.strips + 1), st));
      hipError_t e = sa_launch_long_block(p, st);
      if (e == hipSuccess) e = sa_launch_long_walk(p, st);
      if (e != hipSuccess) return fail_hip(e, "long block / walk launch");
      HIP_TRY(hipMemcpyAsync(h_meta, d_meta, sizeof(LongMeta), hipMemcpyDeviceToHost, st));
      HIP_TRY(stream_wait_spinning(st));
      if (first && h_meta->status != ~0ull) return fail_unknown_pair(pair);   // (NW without a forward pass: its first block is the whole matrix)
      if (h_meta->walk.status) {
        set_last_error("pair " + std::to_string(pair) + ": traceback failed");
        return (int)h_meta->walk.status;
      }
      if (h_meta->walk.done) break;
      if (h_meta->walk.y >= y || h_meta->walk.y != y0) {
        set_last_error("pair " + std::to_string(pair) + ": internal error: the walk left its block at row " + std::to_string(h_meta->walk.y));
        return SEQALIGN_E_HIP;
      }
      x = h_meta->walk.x; y = h_meta->walk.y;
    }

    // the strings home: [head, len_a + len_b)
    const uint32_t head = h_meta->walk.head, n = la + lb - head;
    if ((rc = ctx->h_ta.reserve((uint64_t)n + 16)) || (rc = ctx->h_tb.reserve((uint64_t)n + 16))) return rc;
    if (n) {
      HIP_TRY(hipMemcpyAsync(ctx->h_ta.p, ctx->t_out_a.as<char>() + head, n, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(ctx->h_tb.p, ctx->t_out_b.as<char>() + head, n, hipMemcpyDeviceToHost, st));
      HIP_TRY(stream_wait_spinning(st));
    }
    *len = n;
    *meta = *h_meta;
    *has_alignment = true;
    return SEQALIGN_OK;
  }
};

int long_call(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, bool is_sw, const uint64_t *str_off,
              char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score, const int32_t *min_score, seqalign_sw_hit_t *hits,
              uint64_t hit_cap, uint64_t *n_hits, uint64_t str_cap) {
  int rc;
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, is_sw ? 1 : 0, &sc))) return rc;
  if ((rc = admit_batch(sc, batch, SA_FRAMES_ROWS))) return rc;
  LongPair run{ctx, sc, is_sw};
  HitSink sink{hits, hit_cap, out_a, out_b, str_cap};
  for (uint64_t p = 0; p < batch->n_pairs; ++p) {
    bool has = false;
    uint32_t len = 0;
    LongMeta m;
    if ((rc = run.run(batch, p, is_sw ? min_score[p] : 0, &has, &len, &m))) return rc;
    const char *sa = ctx->h_ta.as<char>(), *sb = ctx->h_tb.as<char>();
    if (!is_sw) {
      memcpy(out_a + str_off[p], sa, len); memcpy(out_b + str_off[p], sb, len);
      out_a[str_off[p] + len] = out_b[str_off[p] + len] = '\0';
      out_len[p] = len;
      out_score[p] = m.walk.end_score;
      continue;
    }
    if (!has) continue;
    const seqalign_sw_hit_t h{p, m.walk.end_score, m.walk.x, m.walk.y, m.walk.end_x - m.walk.x, m.walk.end_y - m.walk.y, len, 0};   // smith_waterman.c:251-255
    const bool fitted = sink.put(ctx, h, sa, sb);
    *n_hits = sink.found;
    if (!fitted) return SEQALIGN_E_NOMEM;
  }
  return SEQALIGN_OK;
}

}  // namespace

extern "C" int seqalign_nw_align_long(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                      const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score) {
  if (!ctx || !scoring || !str_off || !out_a || !out_b || !out_len || !out_score) return SEQALIGN_E_ARG;
  int rc = check_long_batch(batch);
  if (rc) return rc;
  CallScope scope(ctx);
  return long_call(ctx, batch, scoring, false, str_off, out_a, out_b, out_len, out_score, nullptr, nullptr, 0, nullptr, 0);
}

extern "C" int seqalign_sw_align_long(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                      const int32_t *min_score, seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits,
                                      char *out_a, char *out_b, uint64_t str_cap) {
  if (!ctx || !scoring || !min_score || !hits || !n_hits || !out_a || !out_b) return SEQALIGN_E_ARG;
  *n_hits = 0;
  int rc = check_long_batch(batch);
  if (rc) return rc;
  CallScope scope(ctx);
  return long_call(ctx, batch, scoring, true, nullptr, out_a, out_b, nullptr, nullptr, min_score, hits, hit_cap, n_hits, str_cap);
}
