// sa_batch_sw.hip -- seqalign_sw_batch: local alignment over a HOST batch (best hit on the device,
// multi-hit enumeration on the device -- the reverse sweep, sa_sw_sweep.hip -- or the literal host enumeration).
#include "sa_ctx.hpp"

using namespace sa_host;

// ----------------------------------------------- host-level: SW over a batch ---
namespace {

struct Cand { uint32_t idx; int32_t score; };

struct PairHits {
  std::vector<seqalign_sw_hit_t> hits;   // str_off relative to str_a / str_b below
  std::string str_a, str_b;
};


}  // namespace

namespace {

// Successive local alignments of one pair in reference order (score desc, column
// asc, index asc), fresh visited mask, at most max_hits (smith_waterman.c:165-277).
// A high-scoring pair can have tens of thousands of cells above min_score and the
// enumeration usually stops after a few hits, so the candidates are heaped (O(n))
// and popped on demand instead of sorted (upstream sorts ~80 % of ALL cells, :159-161).
static int enumerate_hits(const sa_view_t &v, std::vector<Cand> &cand, uint32_t max_hits, PairHits &out) {
  const size_t W = v.len_a + 1, cells = W * (v.len_b + 1);
  auto later = [W](const Cand &x, const Cand &y) {   // true if x comes AFTER y
    if (x.score != y.score) return x.score < y.score;
    const uint32_t cx = x.idx % W, cy = y.idx % W;
    if (cx != cy) return cx > cy;
    return x.idx > y.idx;
  };
  std::make_heap(cand.begin(), cand.end(), later);
  std::vector<uint32_t> seen((cells + 31) / 32, 0u);
  int rc = SEQALIGN_OK;
  while (!cand.empty() && out.hits.size() < max_hits) {
    std::pop_heap(cand.begin(), cand.end(), later);
    const Cand cd = cand.back();
    cand.pop_back();
    if ((seen[cd.idx >> 5] >> (cd.idx & 31)) & 1u) continue;
    size_t x = cd.idx % W, y = cd.idx / W, steps = 0;
    int matrix = MATCH;
    int32_t score = cd.score;
    bool clash = false;
    for (;; ++steps) {   // pass 1: walk to score 0, marking; abandon on a marked cell
      const size_t at = y * W + x;
      if ((seen[at >> 5] >> (at & 31)) & 1u) { clash = true; break; }
      seen[at >> 5] |= 1u << (at & 31);
      if (score == 0) break;
      if ((rc = sa_reverse_move_rc(&v, &matrix, &score, &x, &y))) return rc;
    }
    if (clash) continue;
    const size_t off = out.str_a.size();
    out.str_a.resize(off + steps + 1);
    out.str_b.resize(off + steps + 1);
    char *ra = &out.str_a[off], *rb = &out.str_b[off];
    x = cd.idx % W; y = cd.idx / W; matrix = MATCH; score = cd.score;
    for (size_t w = steps; score > 0;) {   // pass 2: replay, writing right to left
      --w;
      ra[w] = (matrix == GAP_A) ? '-' : v.a[x - 1];
      rb[w] = (matrix == GAP_B) ? '-' : v.b[y - 1];
      if ((rc = sa_reverse_move_rc(&v, &matrix, &score, &x, &y))) return rc;
    }
    ra[steps] = rb[steps] = '\0';
    seqalign_sw_hit_t h;
    h.pair = 0; h.score = cd.score;
    h.pos_a = (uint32_t)x; h.pos_b = (uint32_t)y;
    h.len_a = (uint32_t)(cd.idx % W - x); h.len_b = (uint32_t)(cd.idx / W - y);
    h.length = (uint32_t)steps; h.str_off = off;
    out.hits.push_back(h);
  }
  return SEQALIGN_OK;
}

}  // namespace


static uint32_t bits_for(uint64_t v) {   // bits needed to hold values 0..v
  uint32_t b = 1;
  while (b < 64 && (v >> b) != 0) ++b;
  return b;
}

// the most one move of an alignment can add to its score (a substitution; a gap only when a gap score is positive --
// legal, absurd)
static int64_t best_move(const seqalign_dev_scoring *sc) {
  const sa_flat_scoring_t &f = sc->flat;
  int64_t best = std::max<int64_t>(1, std::max(f.gen_eq, f.gen_ne));
  for (uint64_t k = 0; k < (uint64_t)f.n_classes * f.n_classes; ++k)
    if (f.table[k] != SA_S_BLOCKED && f.table[k] != SA_S_UNKNOWN) best = std::max<int64_t>(best, f.table[k]);
  return std::max<int64_t>(best, std::max(f.ext, f.open1));
}

// uint64 elements of the multi-hit path's scratch arena a pair needs: the candidate columns of its rows, then its
// hits' keys.  A hit is a walk from a cell with score >= min_score down to score 0, every move takes off at most
// best_move(), and the cells it stands on are won by it alone: ceil(min_score / best move) + 1 cells per hit.
static uint64_t hit_arena_elements(uint32_t len_a, uint32_t len_b, int32_t min_score, int64_t best) {
  const uint64_t cells = ((uint64_t)len_a + 1) * ((uint64_t)len_b + 1);
  const uint64_t per_hit = (uint64_t)((std::max<int64_t>(min_score, 1) + best - 1) / best) + 1;
  return (uint64_t)len_b + 1 + cells / per_hit + 1;
}

// How the sweep packs a cell into a key (SaKeyLayout): row and column fields sized by the longest sequences, the
// score field by the largest score the scoring can produce on them.
static SaKeyLayout key_layout(const seqalign_dev_scoring *sc, uint32_t max_a, uint32_t max_b) {
  const sa_flat_scoring_t &f = sc->flat;
  const int64_t best_step = best_move(sc);
  int64_t cap = (int64_t)std::min(max_a, max_b) * best_step;
  if (f.ext > 0 || f.open1 > 0) cap = ((int64_t)max_a + max_b) * best_step;
  cap = std::min<int64_t>(std::max<int64_t>(cap, 1), INT32_MAX);
  SaKeyLayout l;
  l.cap = (int32_t)cap;
  l.row_bits = bits_for(max_b);
  l.col_bits = bits_for(max_a);
  l.score_bits = bits_for((uint64_t)cap);
  return l;
}
// a key is at most 64 bits wide, all ones excluded
static bool key_layout_fits(const SaKeyLayout &l) { return l.row_bits + l.col_bits + l.score_bits <= 63; }

// ------------------------------------------------- what the chunk functions share ---
namespace {

// The packed two-pairs-per-wave fills' layout of a chunk (sa_fill_dirs_x2.hip), decided once for both SW paths.  stride: 0 -- the
// chunk is not packed; every pair of the chunk the same shape (reads against windows of one length) -- one stride for all, a
// multiple of 256, so that every pair's cells start on one; ragged -- kBucketShapes: run_chunk pairs up the pairs of equal shape,
// every pair on a multiple of 256.  dir_bytes: the direction bytes that layout holds for the chunk (`blocked`: rows in
// the best-hit fill's blocked layout, sa_kernels.h).  min_pairs: from how many same-shape pairs packing pays on this path.
struct PackedShape { uint64_t stride = 0, dir_bytes = 0; };
static PackedShape packed_fill_shape(const seqalign_ctx *ctx, const seqalign_batch_t *batch, const Chunk &c, const seqalign_dev_scoring *sc,
                                     bool (*applicable)(const seqalign_ctx_t *, const seqalign_dev_scoring_t *, uint32_t, uint32_t),
                                     uint64_t min_pairs, bool blocked) {
  const uint64_t n = c.count;
  bool same_shape = true;
  for (uint64_t k = 1; k < n && same_shape; ++k)
    same_shape = batch->len_a[c.first + k] == batch->len_a[c.first] && batch->len_b[c.first + k] == batch->len_b[c.first];
  PackedShape s;
  if (same_shape && (n >= min_pairs || ctx->opt.pack16 == 2) && applicable(ctx, sc, c.max_a, c.max_b)) {
    s.stride = dirs_bytes256(blocked, c.max_a, c.max_b);
    s.dir_bytes = n * s.stride;
  } else if (!same_shape && (n >= kBucketedFillMinPairs || ctx->opt.pack16 == 2) && ((uint64_t)c.max_a + 1) * ((uint64_t)c.max_b + 1) <= kShapeTableMax &&
             applicable(ctx, sc, c.max_a, c.max_b)) {
    s.stride = kBucketShapes;
    for (uint64_t k = 0; k < n; ++k) s.dir_bytes += dirs_bytes256(blocked, batch->len_a[c.first + k], batch->len_b[c.first + k]);
  }
  return s;
}

// Hits that came home as MOVES -- two bit planes per walk in fixed slots of pinned memory (host/sa_moves.c) and four words per
// walk: score, walked columns (or SA_MOVES_ERR | code), end cell x, y -- into the caller's room, for both paths whose walks send
// moves (the packed best-hit call: one walk per pair; the one-trip multi-hit call: max_hits walk slots per pair).
//   h_w, h_moves   the per-walk words and the planes; walk j of pair k is walk k * wpp + j, its planes start at word
//                  2 wpp ((slot[k] >> 5) + k) + 2 j nwd of h_moves (nwd: words per plane of the pair)
//   slot           the prefix of len_a + len_b over the chunk's pairs (run_chunk's packed offsets)
//   walks(k)       how many of pair k's walk slots hold a walk that ran
//   take(k, j)     whether that walk is a hit the caller wants
// Where every hit goes in the caller's buffers: hits and string bytes per block of pairs (parallel -- round 4 counted in one
// serial pass over words the GPU had just written, every line of them a miss: 0.1 ms of C4's 0.89 ms call), a prefix over
// the blocks, then every block places and expands its own hits.  What fits: whole blocks while they do, the first that does not
// hit by hit; SEQALIGN_E_NOMEM is returned AFTER what fits is delivered (as the strings delivery does).  A walk that ran and
// failed is the call's error, the lowest such walk's code (the lowest failing pair's: what the header promises), and nothing
// is delivered then.
template <class Walks, class Take>
static int deliver_moves(seqalign_ctx *ctx, const seqalign_batch_t *batch, const Chunk &c, const uint32_t *h_w, const uint32_t *h_moves,
                         const uint64_t *slot, uint32_t wpp, Walks walks, Take take, HitSink &sink, StageTimer &tm) {
  const uint64_t n = c.count, first = c.first;
  constexpr uint64_t kBlk = 64;    // (pairs per task: C3's 10 000 pairs are 157 tasks for 16-32 threads; 256 left some threads a third more than others)
  const uint64_t nblk = (n + kBlk - 1) / kBlk;
  std::vector<uint64_t> blk_hits_v(nblk + 1, 0), blk_bytes_v(nblk + 1, 0);
  uint64_t *const blk_hits = blk_hits_v.data(), *const blk_bytes = blk_bytes_v.data();
  LowestFailure first_err;   // (of the LOWEST failing walk)
  // The tasks capture what they read per hit BY VALUE, so that the closure's copy on the heap holds it.  Measured (C3, up to 4
  // hits, the placement pass over 10 000 pairs, profiles/r30): 0.19-0.21 ms with everything captured by reference, 0.10-0.13 by
  // value, the parent's copy 0.11-0.12.  The cause is supposed, not shown: after every call into host/sa_moves.c a task reads its
  // constants again, and by reference they lie in this frame, whose lines the calling thread writes next to while it runs tasks.
  auto planes_of = [=](uint64_t k, uint32_t j, uint32_t nwd) { return h_moves + 2ull * wpp * ((slot[k] >> 5) + k) + 2ull * j * nwd; };
  // what hit j of pair k takes in the caller's string buffer: its columns + NUL, or in CIGAR mode (seqalign_sw_batch_cigar) its
  // CIGAR's length + NUL, counted from the planes (host/sa_moves.c)
  auto out_bytes = [=](uint64_t k, uint32_t j, uint32_t len) -> uint64_t {
    if (!ctx->cigar_format) return (uint64_t)len + 1;
    const uint64_t p = first + k, w = k * wpp + j;
    const uint32_t nwd = (batch->len_a[p] + batch->len_b[p] + 31u) >> 5;
    const uint32_t *pa = planes_of(k, j, nwd);
    uint32_t pos[4], clen = 0;
    if (sa_cigar_sw_moves(batch->arena + batch->off_a[p], batch->arena + batch->off_b[p], h_w[4 * w + 2], h_w[4 * w + 3], pa, pa + nwd, nwd, len,
                          ctx->cigar_format, ctx->cigar_fold, nullptr, 0, pos, &clen))
      return 1;   // (the placement pass meets the same error and reports it)
    return (uint64_t)clen + 1;
  };
  parallel_for(nblk, [=, &first_err](uint64_t bi) {
    uint64_t hs = 0, bytes = 0;
    for (uint64_t k = bi * kBlk, e = std::min(n, (bi + 1) * kBlk); k < e; ++k) {
      for (uint32_t j = 0, nj = walks(k); j < nj; ++j) {
        const uint64_t w = k * wpp + j;
        const uint32_t len = h_w[4 * w + 1];
        if (len >= SA_MOVES_ERR) { first_err.note(w, (int)(len & 15u)); continue; }
        if (take(k, j)) { ++hs; bytes += out_bytes(k, j, len); }
      }
    }
    blk_hits[bi + 1] = hs; blk_bytes[bi + 1] = bytes;
  });
  if (first_err.code()) return first_err.code();
  tm.lap("sw moves: hits counted");
  for (uint64_t bi = 0; bi < nblk; ++bi) { blk_hits[bi + 1] += blk_hits[bi]; blk_bytes[bi + 1] += blk_bytes[bi]; }
  const uint64_t hit_room = sink.hit_room(), str_room = sink.str_room();
  const bool out_of_room = blk_hits[nblk] > hit_room || blk_bytes[nblk] > str_room;
  const uint64_t first_hit = sink.found, first_str = sink.used;
  std::atomic<uint64_t> delivered_hits{0}, delivered_bytes{0};
  std::atomic<int> bad{SEQALIGN_OK};
  parallel_for(nblk, [=, &sink, &bad, &delivered_hits, &delivered_bytes](uint64_t bi) {
    uint64_t hi = blk_hits[bi], at = blk_bytes[bi], done_h = 0, done_b = 0;
    if (hi >= hit_room || at >= str_room) return;   // (everything from here on is beyond the caller's room)
    bool stop = false;
    for (uint64_t k = bi * kBlk, e = std::min(n, (bi + 1) * kBlk); k < e && !stop; ++k) {
      if (k + 6 < e) {   // the GPU wrote these lines: every first touch is a miss -- have the pair six ahead on its way
        const uint64_t kn = k + 6;
        const uint32_t nwn = (batch->len_a[first + kn] + batch->len_b[first + kn] + 31u) >> 5;
        const uint32_t *pn = planes_of(kn, 0, nwn);
        __builtin_prefetch(h_w + 4 * kn * wpp); __builtin_prefetch(pn + nwn - 1); __builtin_prefetch(pn + 2 * nwn - 1);
        __builtin_prefetch(batch->arena + batch->off_a[first + kn]);
      }
      const uint64_t p = first + k;
      const uint32_t nwd = (batch->len_a[p] + batch->len_b[p] + 31u) >> 5;
      for (uint32_t j = 0, nj = walks(k); j < nj; ++j) {
        if (!take(k, j)) continue;
        const uint64_t w = k * wpp + j;
        const uint32_t len = h_w[4 * w + 1];
        const uint64_t need = out_bytes(k, j, len);
        if (hi >= hit_room || at + need > str_room) { stop = true; break; }   // (out_of_room is set: the call reports it)
        const uint32_t *pa = planes_of(k, j, nwd);
        uint32_t pos[4], clen = 0;
        const int prc = ctx->cigar_format
          ? sa_cigar_sw_moves(batch->arena + batch->off_a[p], batch->arena + batch->off_b[p], h_w[4 * w + 2], h_w[4 * w + 3], pa, pa + nwd, nwd, len,
                              ctx->cigar_format, ctx->cigar_fold, sink.out_a + first_str + at, need, pos, &clen)
          : sa_expand_sw_moves(batch->arena + batch->off_a[p], batch->arena + batch->off_b[p], h_w[4 * w + 2], h_w[4 * w + 3],
                               pa, pa + nwd, nwd, len, sink.out_a + first_str + at, sink.out_b + first_str + at, pos);
        if (prc) { int expected = SEQALIGN_OK; bad.compare_exchange_strong(expected, prc); stop = true; break; }
        sink.record(first_hit + hi, seqalign_sw_hit_t{p, (int32_t)h_w[4 * w], pos[0], pos[1], pos[2], pos[3], len, 0}, first_str + at);
        ++hi; at += need; ++done_h; done_b += need;
      }
    }
    delivered_hits.fetch_add(done_h, std::memory_order_relaxed); delivered_bytes.fetch_add(done_b, std::memory_order_relaxed);
  });
  sink.used += delivered_bytes.load();
  tm.lap("sw moves: hits expanded");
  if (bad.load()) return bad.load();
  sink.found += delivered_hits.load();
  return out_of_room ? SEQALIGN_E_NOMEM : SEQALIGN_OK;
}

// Hits that came home as STRINGS (walkers that write the two gapped strings into slots of len_a + len_b characters on the
// device), for both paths that have them (the best-hit call off the moves form, the three-trip multi-hit call).  Given nw walks
// with their words at home in h_meta and on the device in dv_meta -- head | len | score | status | pos[4], nw of each -- and
// their string slots' offsets on the device (dv_str_off):
//   a hit is much shorter than its slot of len_a + len_b characters: pack the strings on the device, bring back
//   what was written (C3: 2 x 1.7 MB instead of 2 x 11.5 MB over PCIe),
// then where every wanted hit (take(w, score)) goes in the caller's buffers -- a prefix over the lengths while there is room --
// and the copies and records on the thread pool.  The lowest walk with a status is the call's error; SEQALIGN_E_NOMEM is returned
// after what fits is delivered.  pair_of(w): the batch's pair of walk w.
template <class PairOf, class Take>
static int deliver_strings(seqalign_ctx *ctx, hipStream_t st, uint64_t nw, const uint32_t *h_meta, const uint32_t *dv_meta,
                           const uint64_t *dv_str_off, PairOf pair_of, Take take, HitSink &sink, StageTimer &tm) {
  int rc;
  DevBuf &d_dst = ctx->e[11], &d_gath_a = ctx->e[9];
  std::vector<uint64_t> dst_off(nw);
  uint64_t gathered = 0;
  for (uint64_t w = 0; w < nw; ++w) {
    if (h_meta[3 * nw + w]) return (int)h_meta[3 * nw + w];
    dst_off[w] = gathered;
    gathered += h_meta[nw + w];
  }
  const uint64_t gath_b_at = (gathered + 15) & ~(uint64_t)15;   // a-strings, then b-strings: one buffer, one copy home
  if (nw) {
    if ((rc = d_dst.reserve(nw * 8 + 16)) || (rc = d_gath_a.reserve(gath_b_at + gathered + 16)) ||
        (rc = ctx->h_ta.reserve(gath_b_at + gathered + 16)) || (rc = ctx->h_desc.reserve(nw * 8 + 16)))
      return rc;
    memcpy(ctx->h_desc.p, dst_off.data(), nw * 8);   // (pinned; whatever it held -- run_chunk's descriptors, the walker lists -- is on the device by now: the stream was waited for)
    HIP_TRY(hipMemcpyAsync(d_dst.p, ctx->h_desc.p, nw * 8, hipMemcpyHostToDevice, st));
    const hipError_t e = sa_launch_gather_hits(ctx->t_out_a.as<char>(), ctx->t_out_b.as<char>(), dv_str_off, dv_meta, dv_meta + nw,
                                               d_dst.as<uint64_t>(), d_gath_a.as<char>(), d_gath_a.as<char>() + gath_b_at, (uint32_t)nw, st);
    if (e != hipSuccess) return fail_hip(e, "gather hits");
    HIP_TRY(hipMemcpyAsync(ctx->h_ta.p, d_gath_a.p, gath_b_at + gathered, hipMemcpyDeviceToHost, st));
    HIP_TRY(stream_wait_spinning(st));
  }
  tm.lap("sw strings: gather + strings D2H");
  const char *ha = ctx->h_ta.as<char>(), *hb = ha + gath_b_at;
  auto hit_of = [=](uint64_t w) {
    const uint32_t *pos = h_meta + 4 * nw + 4 * w;
    return seqalign_sw_hit_t{pair_of(w), reinterpret_cast<const int32_t *>(h_meta)[2 * nw + w], pos[0], pos[1], pos[2], pos[3], h_meta[nw + w], 0};
  };
  struct Placed { uint64_t walk, str_off; };
  std::vector<Placed> placed;
  const uint64_t first_hit = sink.found;
  bool no_room = false;
  for (uint64_t w = 0; w < nw; ++w) {
    const uint32_t len = h_meta[nw + w];
    if (!take(w, reinterpret_cast<const int32_t *>(h_meta)[2 * nw + w])) continue;
    if (ctx->cigar_format) {   // CIGAR mode on a path whose walkers write strings: encode them, one after the other (not the common kind)
      if (!sink.put(ctx, hit_of(w), ha + dst_off[w], hb + dst_off[w])) { no_room = true; break; }
      continue;
    }
    if (!sink.hit_room() || (uint64_t)len + 1 > sink.str_room()) { no_room = true; break; }
    placed.push_back(Placed{w, sink.used});
    ++sink.found; sink.used += (uint64_t)len + 1;
  }
  constexpr uint64_t kPack = 1024;
  const Placed *const pl = placed.data();
  const uint64_t n_placed = placed.size(), *const src_off = dst_off.data();
  parallel_for((n_placed + kPack - 1) / kPack, [=, &sink](uint64_t blk) {   // (by value: see deliver_moves)
    for (uint64_t i = blk * kPack, e = std::min(n_placed, (blk + 1) * kPack); i < e; ++i) {
      const uint64_t w = pl[i].walk, at = pl[i].str_off;
      const uint32_t len = h_meta[nw + w];
      memcpy(sink.out_a + at, ha + src_off[w], len);
      memcpy(sink.out_b + at, hb + src_off[w], len);
      sink.out_a[at + len] = sink.out_b[at + len] = '\0';
      sink.record(first_hit + i, hit_of(w), at);
    }
  });
  tm.lap("sw strings: unpack hits");
  return no_room ? SEQALIGN_E_NOMEM : SEQALIGN_OK;
}

// SW hits of one chunk, enumerated on the device:
//   fill (reports the candidates' count, box and columns per row) -> reverse sweep (sa_sw_sweep.hip: every hit's
//   key, in order)
//   -> one traceback per wanted hit -> strings packed -> D2H.
// Host round trips: the hit counts (they size the traceback), the hits' lengths (they size the packing), the strings -- or ONE
// trip for everything when the call is the common kind (enqueue).  Appends to the caller's hit array / string buffers.
// plan (sizes, scratch, which fill) -> enqueue (fill, sweep, with luck the walks) -> finish_one_trip | finish_three_trip.
struct SwEnumChunk {
  seqalign_ctx *ctx;
  const seqalign_batch_t *batch;
  const Chunk &c;
  const seqalign_dev_scoring *sc;
  const int32_t *min_score;
  const uint32_t max_hits;
  HitSink &sink;
  const uint64_t n;
  hipStream_t st;
  DevBuf &d_min, &d_keys, &d_box, &d_rows, &d_rowoff, &d_walk, &d_hits, &d_meta, &d_hitoff, &d_trace;
  // sources of asynchronous H2D copies: declared BEFORE the guard below, so that they are destroyed after its
  // hipStreamSynchronize on every exit path
  std::vector<uint64_t> hit_off, row_off, walk_str;
  std::vector<uint32_t> walk_pair, walk_rank;
  StreamSyncOnExit sync_on_exit;
  StageTimer tm;
  const SaKeyLayout layout;
  const bool trace;   // development aid: per-pair counters on stderr
  SaCandBox cand{};
  SaSweepParams q;
  seqalign_dev_batch_t d;
  bool dirs_used = false, allow_dirs = false, may_one_trip = false, one_trip = false;
  uint64_t stride = 0;

  SwEnumChunk(seqalign_ctx *ctx_, const seqalign_batch_t *batch_, const Chunk &c_, const seqalign_dev_scoring *sc_, const int32_t *min_score_,
              uint32_t max_hits_, HitSink &sink_)
      : ctx(ctx_), batch(batch_), c(c_), sc(sc_), min_score(min_score_), max_hits(max_hits_), sink(sink_), n(c_.count), st(ctx_->stream),
        d_min(ctx_->e[0]), d_keys(ctx_->e[1]), d_box(ctx_->e[3]), d_rows(ctx_->e[4]), d_rowoff(ctx_->e[5]), d_walk(ctx_->e[6]),
        d_hits(ctx_->e[7]), d_meta(ctx_->e[8]), d_hitoff(ctx_->e[13]), d_trace(ctx_->e[12]), hit_off(c_.count + 1, 0), sync_on_exit(ctx_->stream),
        tm(ctx_->opt.timing), layout(key_layout(sc_, c_.max_a, c_.max_b)), trace(ctx_->opt.sweep_trace) {
    memset(&q, 0, sizeof(q));
  }
  SwEnumChunk(const SwEnumChunk &) = delete;   // (cand points into it)

  SaSweepParams sweep_params(bool dirs) const {
    SaSweepParams r;
    memset(&r, 0, sizeof(r));
    r.arena = d.arena; r.off_a = d.off_a; r.len_a = d.len_a; r.off_b = d.off_b; r.len_b = d.len_b;
    r.mat_off = d.mat_off; r.M = d.match_scores; r.A = d.gap_a_scores; r.B = d.gap_b_scores;
    r.code = sc->d_code; r.table = sc->d_table; r.cand_count = cand.cand_count; r.cand_box = cand.cand_box;
    r.min_score = d_min.as<int32_t>(); r.hit_keys = d_keys.as<unsigned long long>(); r.hit_off = d_hitoff.as<uint64_t>();
    r.err_key = d_meta.as<unsigned long long>();
    r.hit_count = reinterpret_cast<uint32_t *>(d_meta.as<unsigned long long>() + n); r.status = r.hit_count + n;
    r.n_pairs = (uint32_t)n; r.K = sc->flat.n_classes; r.open1 = sc->flat.open1; r.ext = sc->flat.ext;
    r.gen_eq = sc->flat.gen_eq; r.gen_ne = sc->flat.gen_ne; r.flags = sc->flat.flags;
    r.max_len_a = c.max_a; r.max_len_b = c.max_b; r.layout = layout; r.tune_cpl = ctx->opt.sweep_cpl; r.tune_ev = ctx->opt.sweep_ev;
    r.dirs = dirs ? cand.dirs : nullptr;
    return r;
  }

  // ---- sizes and scratch; which fill, and whether everything may go in one trip
  int plan() {
    int rc;
    if (!key_layout_fits(layout)) return SEQALIGN_E_TOO_LARGE;   // (seqalign_sw_batch checks the whole batch first)
    // every pair's part of the scratch arena (its rows' candidate columns, then its hits' keys)
    {
      const int64_t best = best_move(sc);
      uint32_t pa = ~0u, pb = ~0u; int32_t pm = 0; uint64_t pe = 0;   // (reads of one length: the division once per run of equal pairs)
      for (uint64_t k = 0; k < n; ++k) {
        const uint32_t xa = batch->len_a[c.first + k], xb = batch->len_b[c.first + k];
        const int32_t xm = min_score[c.first + k];
        if (xa != pa || xb != pb || xm != pm) { pa = xa; pb = xb; pm = xm; pe = hit_arena_elements(xa, xb, xm, best); }
        hit_off[k + 1] = hit_off[k] + pe;
      }
    }
    if ((rc = d_min.reserve(n * 4)) || (rc = ctx->cand_count.reserve(n * 4)) || (rc = d_box.reserve(n * 16)) ||
        (rc = d_keys.reserve(hit_off[n] * 8 + 16)) || (rc = d_meta.reserve(n * 16 + 16)) || (rc = d_hitoff.reserve((n + 1) * 8)))
      return rc;
    // (from pinned staging: a copy from the caller's pageable array is staged by the runtime and waited for)
    if ((rc = ctx->h_tb.reserve((n + 1) * 8 + n * 4 + 16))) return rc;
    { uint64_t *hs_off = ctx->h_tb.as<uint64_t>();
      int32_t *hs_min = reinterpret_cast<int32_t *>(hs_off + n + 1);
      memcpy(hs_off, hit_off.data(), (n + 1) * 8); memcpy(hs_min, min_score + c.first, n * 4);
      HIP_TRY(hipMemcpyAsync(d_hitoff.p, hs_off, (n + 1) * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_min.p, hs_min, n * 4, hipMemcpyHostToDevice, st)); }
    cand.cand_count = ctx->cand_count.as<uint32_t>(); cand.cand_box = d_box.as<uint32_t>(); cand.cand_min = d_min.as<int32_t>();
    cand.cand_rows = d_keys.as<uint32_t>(); cand.hit_off = d_hitoff.as<uint64_t>();
    // plain scorings, rows up to 1 024 columns (513 and up: see wide_ok below): the fill writes match_scores + one byte of directions per cell instead of the
    // three matrices (sa_fill_dirs.hip); the directions go where gap_a_scores would have gone
    // every pair of the chunk the same shape (reads against windows of one length), match / mismatch scoring: the packed
    // two-pairs-per-wave fill (sa_fill_dirs_x2.hip); every pair's cells then start on a multiple of 256
    const PackedShape shape = packed_fill_shape(ctx, batch, c, sc, sw_dirs_x2_applicable, kPackedFillMinPairs, false);
    stride = shape.stride;
    // (only when the sweep will run in its rows-in-registers form: not with the strip / LDS forms forced by an option)
    // and rows of 513 .. 1 024 columns only where the sweep's one-word form takes them (sa_launch_sw_sweep) and a wave per pair fills
    // the chip (few wide pairs: strips, below, as before)
    const bool wide_row = c.max_a + 1 > 512;
    const bool wide_ok = ctx->opt.sweep_ev && layout.row_bits + layout.col_bits + layout.score_bits <= 62 &&
                         (n >= (c.max_a + 1 > 768 ? 640u : 128u) || ctx->opt.sweep_mode == 1);
    // (tools/sw_wide_few.py, 700 x 1000 -- 12 columns per lane: 128 pairs 4.04 -> 3.69 ms, 64: 3.51 -> 3.67; 900 x 1000 -- 16 per lane:
    //  512 pairs 5.8 on strips / 6.3 here, 1 024 pairs 8.1 / 6.2)
    allow_dirs = ctx->opt.sweep_mode != 2 && ctx->opt.sweep_cpl == 0 && (!wide_row || wide_ok);
    // (the packed direction-byte fill is bound by instruction issue: its arenas need no placement walk)
    if ((rc = reserve_arenas(ctx, (stride ? shape.dir_bytes : c.cells) * 4, !(allow_dirs && stride != 0)))) return rc;
    cand.dirs = allow_dirs ? ctx->A.as<uint8_t>() : nullptr; cand.dirs_used = &dirs_used;
    if (!allow_dirs) stride = 0;
    cand.uniform_stride = stride == kBucketShapes ? 256 : stride;
    may_one_trip = allow_dirs && ctx->opt.sweep_mode == 0 && !trace && ctx->opt.nw_moves && max_hits <= 8 &&
                   n * max_hits <= ((uint64_t)4 << 20) && c.max_a + 1 <= 1024;
    if (may_one_trip) {
      const uint64_t move_words = 2ull * max_hits * ((c.seq_bytes >> 5) + n) + 2;
      if ((rc = ctx->h_ta.reserve(move_words * 4)) || (rc = ctx->h_B.reserve(n * max_hits * 16 + 16)) || (rc = ctx->h_tmeta.reserve(n * 16 + 64)))   // (h_misc is fetch_status')
        return rc;
    }
    return SEQALIGN_OK;
  }

  // ---- the fill, the sweep -- every hit of every pair -- and, when the call is the common kind, the walks
  int enqueue() {
    int rc;
    hipError_t e;
    bool reported = false;
    if ((rc = run_chunk(ctx, batch, c, sc, &d, nullptr, &cand, &reported, stride))) return rc;
    // ---- ONE trip for everything, when the call is the common kind: direction bytes, one wave per pair in the sweep, a few
    // hits per pair wanted.  The hit walks are launched BEFORE anybody has seen the sweep's counts -- max_hits walks per pair,
    // walk w = hit w % max_hits of pair w / max_hits, those beyond a pair's hits return at once (sa_traceback.hip) -- and send
    // home two bits per column into fixed slots of pinned memory (host/sa_moves.c), so nothing has to be sized, gathered or
    // copied by a second and third launch + wait: counts, per-walk words and moves are all there after one synchronisation,
    // and the host threads expand the hits straight into the caller's buffers.  (Round 3: counts -> walker lists -> walks ->
    // lengths -> gather -> strings, three waits.)  Sweep and walks follow the chunk's last fill, in the fills' stream.
    // (Measured, profiles/r04/r04_sw_pipeline.txt: on a second stream, with equal slices so that a slice's sweep runs beside
    // the next slice's fill -- both issue vector instructions 50-70 % of the time, neither is bound by memory -- the two
    // kernels simply share the SIMDs: C3's sweep of 4 096 pairs 0.62 -> 1.97 ms beside a fill, the call 4.6 -> 5.4 ms; and a
    // sweep on the second, high-priority stream alone behind an event starts 80 us late and runs 0.93 instead of 0.80 ms on C4.)
    // A pair that needs the host between sweep and walks -- more than 64 hits (keys unsorted), an error to weigh against
    // max_hits -- sends the whole chunk down the three-trip path, which starts from the same counts.
    // (behind ALL the fills: per slice -- a small first slice's sweep and walks, then the rest's -- C3 took 5.2 instead of 4.7 ms)
    one_trip = may_one_trip && dirs_used && reported;   // (else not the common kind: the three-trip path, for the whole chunk)
    if (one_trip) {
      q = sweep_params(true);
      if ((e = sa_launch_sw_sweep(q, st)) != hipSuccess) return fail_hip(e, "sw sweep");
      SaTraceParams t = trace_params(ctx, sc, d);
      t.M = d.match_scores;
      t.str_off = d.off_a;                       // (run_chunk packs a, b, a, b, ...: off_a IS the prefix of len_a + len_b)
      // walk w of the launch is hit w % max_hits of pair w / max_hits: its slot is 2 max_hits ((off_a >> 5) + pair) + ...
      t.stage_words = (c.max_a + c.max_b + 31u) >> 5;
      t.moves = ctx->h_ta.dev_as<uint32_t>(); t.out_meta4 = ctx->h_B.dev_as<uint32_t>();
      t.walks_per_pair = max_hits; t.hit_count = q.hit_count; t.sweep_status = q.status;
      t.hit_keys = q.hit_keys; t.hit_off = q.hit_off; t.layout = layout; t.fill_status = d.status;
      t.n_pairs = (uint32_t)(n * max_hits); t.dirs = q.dirs;
      if ((e = sa_launch_nw_traceback(t, st)) != hipSuccess) return fail_hip(e, "sw hit traceback");
      // everything is enqueued on the one stream: one wait for all of it
      tm.lap("sw: fills, sweeps, walks enqueued");
      return SEQALIGN_OK;
    }
    if (!reported) {   // a fill kernel that cannot report them itself: one pass over match_scores
      SaReduceParams r;
      memset(&r, 0, sizeof(r));
      r.len_a = d.len_a; r.len_b = d.len_b; r.mat_off = d.mat_off; r.M = d.match_scores; r.n_pairs = (uint32_t)n;
      if ((e = sa_launch_sw_box(r, cand, c.max_b, st)) != hipSuccess) return fail_hip(e, "sw candidate box");
    }
    q = sweep_params(dirs_used);
    // How the pairs are laid over waves (sa_sw_sweep.hip): one wave per pair -- rows in registers (up to 512 columns on three matrices, up to 1 024 on direction bytes),
    // wider ones in segments with the winners of two rows in LDS -- or, for FEW wide pairs (a wave per pair would leave
    // the chip empty) and for rows too wide for LDS, one wave per 256-column strip.  The option sweep_mode = strips | pair
    // forces one (tests, experiments).
    const int mode_opt = ctx->opt.sweep_mode;   // 0 auto, 1 pair, 2 strips
    const uint32_t w_max = c.max_a + 1;
    bool strips = !dirs_used && c.max_a + 1 > 512 && (c.max_a + 1 > SA_SWEEP_LDS_COLUMNS || n < 1024);
    if (mode_opt == 2) strips = true;
    if (mode_opt == 1 && w_max <= SA_SWEEP_LDS_COLUMNS) strips = false;
    if (w_max <= SA_SWEEP_LDS_COLUMNS) q.lds_columns = (c.max_a + 2u) & ~1u;
    DevBuf &d_prog = ctx->e[2];
    if (strips) {
      // strip width by how many waves that makes: 128-column strips (and progress published every 16 rows instead of
      // 64) when the pairs are so few that 256-column strips would leave most of the chip idle (2 x 10 000^2: 42.7 ->
      // 32.8 ms; 64-column strips gain nothing more: a row's dependent passes cost ~2 us whatever its width)
      uint32_t cols = sa_sweep_strip_blocks((uint32_t)n, c.max_a, 256) < 1024 ? 128 : 256;
      if (const uint32_t v = ctx->opt.sweep_strip; v == 64 || v == 128 || v == 256) cols = v;
      q.strip_columns = cols; q.strip_interval = cols == 256 ? 64 : 16;
      const uint32_t spp = sa_sweep_strips_per_pair(c.max_a, cols);
      const uint64_t blocks = sa_sweep_strip_blocks((uint32_t)n, c.max_a, cols);
      row_off.resize(n);
      uint64_t rows_total = 0;
      for (uint64_t k = 0; k < n; ++k) { row_off[k] = rows_total; rows_total += (uint64_t)batch->len_b[c.first + k] + 1; }
      if ((rc = d_prog.reserve((2 * blocks + 1) * 4 + 16)) || (rc = d_rows.reserve(rows_total * spp * 16 + 16)) ||
          (rc = d_rowoff.reserve(n * 8)))
        return rc;
      HIP_TRY(hipMemsetAsync(d_prog.p, 0, (2 * blocks + 1) * 4, st));
      HIP_TRY(hipMemsetAsync(q.err_key, 0xff, n * 8, st));     // the strips of a pair report into the same words
      HIP_TRY(hipMemsetAsync(q.hit_count, 0, n * 8, st));      // hit_count | status
      HIP_TRY(hipMemcpyAsync(d_rowoff.p, row_off.data(), n * 8, hipMemcpyHostToDevice, st));
      q.strip_progress = d_prog.as<uint32_t>(); q.strips_per_pair = spp;
      q.bnd = d_rows.as<unsigned long long>(); q.row_off = d_rowoff.as<uint64_t>();
    }
    if (trace) {
      if ((rc = d_trace.reserve(n * 64))) return rc;
      HIP_TRY(hipMemsetAsync(d_trace.p, 0, n * 64, st));
      q.trace = d_trace.as<unsigned long long>();
    }
    if ((e = sa_launch_sw_sweep(q, st)) != hipSuccess) return fail_hip(e, "sw sweep");
    tm.lap("sw: enqueue fill + sweep");
    return SEQALIGN_OK;
  }

  // ---- the one trip's end: counts, per-walk words and moves are at home after one wait.  *clean = false: a pair needs the
  // host between sweep and walks, the chunk goes the three-trip way (nothing was delivered)
  int finish_one_trip(bool *clean) {
    int rc;
    unsigned long long *h_err = ctx->h_tmeta.as<unsigned long long>();
    const uint32_t *h_cnt = reinterpret_cast<const uint32_t *>(h_err + n), *h_st = h_cnt + n;
    HIP_TRY(hipMemcpyAsync(h_err, d_meta.p, n * 16, hipMemcpyDeviceToHost, st));
    if ((rc = fetch_status(ctx, c, nullptr))) return rc;   // the fill's status words; synchronises the stream
    tm.lap("sw one trip: wait (fill, sweep, walks)");
    *clean = true;
    for (uint64_t k = 0; k < n && *clean; ++k) *clean = h_st[k] == 0;
    tm.lap("sw one trip: statuses checked");
    if (!*clean) return SEQALIGN_OK;
    // (run_chunk's packed offsets: the prefix of len_a + len_b over the chunk's pairs, in the pinned descriptor block)
    const uint32_t wpp = max_hits;
    return deliver_moves(ctx, batch, c, ctx->h_B.as<uint32_t>(), ctx->h_ta.as<uint32_t>(), ctx->h_desc.as<uint64_t>(), wpp,
                         [=](uint64_t k) { return std::min(h_cnt[k], wpp); }, [](uint64_t, uint32_t) { return true; }, sink, tm);
  }

  // ---- three trips: the hit counts (with the rare cases the host settles: a pair's unsorted keys, an error that max_hits
  // makes moot), one traceback per wanted hit and its lengths, the strings
  int finish_three_trip() {
    int rc;
    // ---- round trip 1: hit counts and status
    if ((rc = ctx->h_tmeta.reserve(n * 16 + 64))) return rc;
    unsigned long long *h_err_key = ctx->h_tmeta.as<unsigned long long>();
    const uint32_t *h_count = reinterpret_cast<const uint32_t *>(h_err_key + n), *h_status = h_count + n;
    HIP_TRY(hipMemcpyAsync(h_err_key, d_meta.p, n * 16, hipMemcpyDeviceToHost, st));
    if ((rc = fetch_status(ctx, c, nullptr))) return rc;   // fill status; synchronises the stream
    tm.lap("sw: wait (fill + sweep), counts");
    if (trace) {
      std::vector<unsigned long long> t(8 * n);
      HIP_TRY(hipMemcpyAsync(t.data(), d_trace.p, n * 64, hipMemcpyDeviceToHost, st));
      HIP_TRY(stream_wait_spinning(st));
      double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hits_total = 0;
      for (uint64_t k = 0; k < n; ++k) {
        for (int j = 0; j < 8; ++j) sum[j] += (double)t[8 * k + j];
        hits_total += h_count[k];
      }
      fprintf(stderr, "[seqalign sweep trace] pairs %llu  per pair: %.0f cycles (s_memtime), %.1f rows, %.1f active row segments, "
                      "%.1f passes, %.0f cycles in active segments, %.2f hits; wide pairs, per row: prefetch issue %.0f, segments %.0f, fence + rotate %.0f cycles\n",
              (unsigned long long)n, sum[0] / n, sum[1] / n, sum[2] / n, sum[3] / n, sum[4] / n, hits_total / n, sum[5] / n, sum[6] / n, sum[7] / n);
    }

    uint64_t str_total = 0;
    bool overflow = false;
    std::vector<unsigned long long> big;
    for (uint64_t k = 0; k < n && !overflow; ++k) {
      const uint32_t cnt = h_count[k], take = std::min(cnt, max_hits);
      unsigned long long *dev_keys = d_keys.as<unsigned long long>() + hit_off[k] + batch->len_b[c.first + k] + 1;
      if (h_status[k] & SA_SWEEP_UNSORTED) {   // more than 64 hits in one pair: ordered here (rare; that pair's keys only)
        // (on the context's stream, waited for both ways: the kernels that wrote the keys and the walkers that read them
        // run on that stream, and it is a non-blocking one -- a null-stream hipMemcpy would not be ordered with it)
        big.resize(cnt);
        HIP_TRY(hipMemcpyAsync(big.data(), dev_keys, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(stream_wait_spinning(st));
        std::sort(big.begin(), big.end());
        HIP_TRY(hipMemcpyAsync(dev_keys, big.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(stream_wait_spinning(st));
      }
      if (h_status[k] & SA_SWEEP_OVERFLOW) {
        set_last_error("seqalign_sw_batch: internal error: pair " + std::to_string(c.first + k) + " has more hits than its share of the scratch arena");
        return SEQALIGN_E_HIP;
      }
      if (const uint32_t err = h_status[k] & ~SA_SWEEP_UNSORTED) {
        // a walk met an error.  The reference would have met it too unless it had stopped before: max_hits hits
        // found among the walks in front of this one
        bool moot = false;
        if (cnt >= max_hits) {
          unsigned long long last;
          HIP_TRY(hipMemcpyAsync(&last, dev_keys + (max_hits - 1), 8, hipMemcpyDeviceToHost, st));
          HIP_TRY(stream_wait_spinning(st));
          moot = last < h_err_key[k];
        }
        if (!moot) return (int)err;
      }
      const uint64_t slot = (uint64_t)batch->len_a[c.first + k] + batch->len_b[c.first + k];
      for (uint32_t j = 0; j < take; ++j) {
        if (sink.found + walk_pair.size() >= sink.hit_cap) { overflow = true; break; }   // reported after what fits is delivered
        walk_pair.push_back((uint32_t)k); walk_rank.push_back(j); walk_str.push_back(str_total);
        str_total += slot;
      }
    }
    const uint64_t nw = walk_pair.size();
    if (nw > 0xffffffffull) return SEQALIGN_E_TOO_LARGE;

    // ---- one traceback per hit (smith_waterman.c:217-255; the traceback kernels of sa_traceback.hip, one walk per hit)
    // per walk: head | len | score | status | pos[4]
    if ((rc = d_walk.reserve(nw * 16 + 16)) || (rc = d_hits.reserve(nw * 32 + 16)) ||
        (rc = ctx->t_out_a.reserve(str_total + 16)) || (rc = ctx->t_out_b.reserve(str_total + 16)) ||
        (rc = ctx->h_misc.reserve(nw * 32 + 16)))
      return rc;
    uint64_t *dv_walk_str = d_walk.as<uint64_t>();
    uint32_t *dv_walk_pair = reinterpret_cast<uint32_t *>(dv_walk_str + nw), *dv_walk_rank = dv_walk_pair + nw;
    uint32_t *dv_meta = d_hits.as<uint32_t>();
    if (nw) {
      // the three lists as the one block they are on the device, from pinned memory: one copy instead of three staged ones
      if ((rc = ctx->h_desc.reserve(nw * 16 + 16))) return rc;
      { uint64_t *hw_str = ctx->h_desc.as<uint64_t>();
        uint32_t *hw_pair = reinterpret_cast<uint32_t *>(hw_str + nw), *hw_rank = hw_pair + nw;
        memcpy(hw_str, walk_str.data(), nw * 8); memcpy(hw_pair, walk_pair.data(), nw * 4); memcpy(hw_rank, walk_rank.data(), nw * 4);
        HIP_TRY(hipMemcpyAsync(dv_walk_str, hw_str, nw * 16, hipMemcpyHostToDevice, st)); }
      SaTraceParams t = trace_params(ctx, sc, d);
      t.M = d.match_scores; t.A = d.gap_a_scores; t.B = d.gap_b_scores;
      t.str_off = dv_walk_str;
      t.out_a = ctx->t_out_a.as<char>(); t.out_b = ctx->t_out_b.as<char>();
      t.out_head = dv_meta; t.out_len = dv_meta + nw; t.out_score = reinterpret_cast<int32_t *>(dv_meta + 2 * nw);
      t.trace_status = dv_meta + 3 * nw; t.out_pos = dv_meta + 4 * nw;
      t.walker_pair = dv_walk_pair; t.walker_rank = dv_walk_rank; t.hit_keys = q.hit_keys; t.hit_off = q.hit_off; t.layout = layout;
      t.n_pairs = (uint32_t)nw; t.dirs = q.dirs;
      const hipError_t e = sa_launch_nw_traceback(t, st);
      if (e != hipSuccess) return fail_hip(e, "sw hit traceback");
      // ---- round trip 2: the hits (their lengths size the packing)
      HIP_TRY(hipMemcpyAsync(ctx->h_misc.p, dv_meta, nw * 32, hipMemcpyDeviceToHost, st));
      HIP_TRY(stream_wait_spinning(st));
    }
    tm.lap("sw: hit tracebacks");
    // ---- round trip 3: the strings
    const uint64_t first = c.first;
    const uint32_t *pair_in_chunk = walk_pair.data();
    if ((rc = deliver_strings(ctx, st, nw, ctx->h_misc.as<uint32_t>(), dv_meta, dv_walk_str,
                              [=](uint64_t w) { return first + pair_in_chunk[w]; }, [](uint64_t, int32_t) { return true; }, sink, tm)))
      return rc;
    return overflow ? SEQALIGN_E_NOMEM : SEQALIGN_OK;
  }
};

static int sw_chunk_device_enumerate(seqalign_ctx *ctx, const seqalign_batch_t *batch, const Chunk &c, const seqalign_dev_scoring *sc,
                                     const int32_t *min_score, uint32_t max_hits, HitSink &sink) {
  SwEnumChunk s(ctx, batch, c, sc, min_score, max_hits, sink);
  int rc;
  if ((rc = s.plan()) || (rc = s.enqueue())) return rc;
  if (s.one_trip) {
    bool clean = false;
    if ((rc = s.finish_one_trip(&clean)) || clean) return rc;
  }
  return s.finish_three_trip();
}

// best hit of every pair of one chunk: fill (+ best cell) -> device traceback -> the hits home as moves or as strings
static int sw_chunk_best_hit(seqalign_ctx *ctx, const seqalign_batch_t *batch, const Chunk &c,
                             const seqalign_dev_scoring *sc, const int32_t *min_score, HitSink &sink) {
  int rc;
  seqalign_dev_batch_t d;
  bool have_best = false;   // the stream kernel reports the best cell itself
  const uint64_t n = c.count;
  StageTimer tm(ctx->opt.timing);
  // Every pair of the chunk the same shape, match / mismatch scoring, scores inside int16: the fill writes only a byte of
  // directions per cell and finds the best cell itself, two pairs per wave (sa_fill_dirs_x2.hip: fill_sw_best_x2_kernel);
  // the walk follows the bytes.  No match_scores, no gap matrices: they are not even allocated.
  bool dirs_used = false;
  // (the walks below as tile walks sending home moves: the fill writes the direction byte's LOCAL form, sa_kernels.h)
  // (whatever the chunk's size: 26 000-40 000 pairs of configs[2]'s / [3]'s shape are 0-9 % faster with tile walks on the local form than with
  //  lane walks on the older one: profiles/r06/r06_local_dirs.txt)
  const bool local = ctx->opt.dirs_local && ctx->opt.nw_moves && (ctx->opt.trace_kernel ? ctx->opt.trace_kernel == 2 : true);
  // From how many pairs: what this fill competes with below that is not a one-pair direction fill (the NW / multi-hit paths'
  // kPackedFillMinPairs) but three matrices and their walker.  tools/sw_best_few.py, same process, packed against not:
  // BLOSUM62 300 x 300 -- ahead at every size (128 pairs 0.52 -> 0.46 ms, 2 047 pairs 0.92 -> 0.58); match / mismatch, 150 x 1 000 --
  // level at ~1 400 pairs (1 024: 0.68 -> 0.76, 2 047: 0.99 -> 0.83); 700 x 1 000 -- at ~700 (512: 1.63 -> 1.94, 1 024: 2.25 -> 2.00,
  // 2 047: 4.10 -> 2.11): a wave's row costs more with two pairs in it, which is what a launch too small to fill the chip pays.
  const uint64_t best_min_pairs = sc->flat.n_classes > 1 ? 128 : c.max_a + 1 > 512 ? 1024 : 1536;
  const PackedShape shape = packed_fill_shape(ctx, batch, c, sc, sw_best_x2_applicable, best_min_pairs, sa_dirs_blocked_shape(c.max_a));
  if (shape.stride) {
    if ((rc = ctx->dirs.reserve(shape.dir_bytes + 4096))) return rc;
    SaCandBox bc;
    memset(&bc, 0, sizeof(bc));
    bc.dirs = ctx->dirs.as<uint8_t>(); bc.dirs_used = &dirs_used; bc.best_only = true; bc.dirs_local = local;
    bc.uniform_stride = shape.stride == kBucketShapes ? 256 : shape.stride;
    if ((rc = run_chunk(ctx, batch, c, sc, &d, &have_best, &bc, nullptr, shape.stride))) return rc;
    if (!dirs_used || !have_best) { set_last_error("seqalign_sw_batch: internal error: the best-hit direction fill did not run"); return SEQALIGN_E_HIP; }
  } else if ((rc = run_chunk(ctx, batch, c, sc, &d, &have_best))) {
    return rc;
  }
  if (!have_best) {
    if ((rc = ctx->best_score.reserve(n * 4)) || (rc = ctx->best_index.reserve(n * 8))) return rc;
    SaReduceParams r;
    memset(&r, 0, sizeof(r));
    r.n_pairs = (uint32_t)n; r.len_a = d.len_a; r.len_b = d.len_b; r.mat_off = d.mat_off; r.M = d.match_scores;
    r.min_score = 1; r.best_score = ctx->best_score.as<int32_t>(); r.best_index = ctx->best_index.as<uint64_t>();
    // few long pairs: several waves per pair (a wave streams ~4 GB/s on its own)
    const uint64_t max_cells = ((uint64_t)c.max_a + 1) * ((uint64_t)c.max_b + 1);
    if (n < 2048) r.slices = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(max_cells >> 18, 1), 4096);
    hipError_t e = sa_launch_sw_reduce(r, ctx->stream);
    if (e != hipSuccess) return fail_hip(e, "sw reduce launch");
  }
  if ((rc = ctx->h_tmeta.reserve(n * 8 + n * 32))) return rc;
  uint64_t *h_off = ctx->h_tmeta.as<uint64_t>();
  uint64_t total = 0;
  for (uint64_t k = 0; k < n; ++k) {
    h_off[k] = total;
    total += (uint64_t)batch->len_a[c.first + k] + batch->len_b[c.first + k];
  }
  if ((rc = ctx->t_str_off.reserve(n * 8)) || (rc = ctx->t_out_a.reserve(total + 16)) ||
      (rc = ctx->t_out_b.reserve(total + 16)) || (rc = ctx->t_meta.reserve(n * 32)))
    return rc;
  hipStream_t st = ctx->stream;
  StreamSyncOnExit sync_on_exit(st);
  HIP_TRY(hipMemcpyAsync(ctx->t_str_off.p, h_off, n * 8, hipMemcpyHostToDevice, st));
  const uint64_t first = c.first;
  if (dirs_used && ctx->opt.nw_moves) {
    // the walk sends home two bits per column into the pair's slot of pinned memory, the host expands (as seqalign_nw_batch):
    // one launch, one wait -- no lengths to fetch before a gather, no gather, no strings over PCIe
    const uint64_t move_words = 2ull * ((total >> 5) + n) + 2;
    if ((rc = ctx->h_ta.reserve(move_words * 4)) || (rc = ctx->h_B.reserve(n * 16 + 16))) return rc;   // (h_misc is fetch_status')
    SaTraceParams tp = trace_params(ctx, sc, d);
    tp.str_off = d.off_a;
    tp.stage_words = (c.max_a + c.max_b + 31u) >> 5;
    tp.moves = ctx->h_ta.dev_as<uint32_t>(); tp.out_meta4 = ctx->h_B.dev_as<uint32_t>();
    tp.start_index = ctx->best_index.as<uint64_t>(); tp.start_score = ctx->best_score.as<int32_t>();
    tp.dirs = ctx->dirs.as<uint8_t>(); tp.dirs_blocked = sa_dirs_blocked_shape(c.max_a); tp.dirs_local = local; tp.tune_stage = ctx->opt.walk_stage; tp.tune_tile = ctx->opt.walk_tile; tp.fill_status = d.status;
    tp.n_pairs = (uint32_t)n;
    hipError_t e2 = sa_launch_nw_traceback(tp, st);
    if (e2 != hipSuccess) return fail_hip(e2, "sw best-hit traceback");
    tm.lap("sw best hit: fill + walk enqueued");
    // (no fetch_status here: a direction fill is only admitted for scorings in which every character pair has a score, and the
    // walks carry a pair's fill status home in their own word anyway -- the copy and its scan were 20 us of nothing)
    HIP_TRY(stream_wait_spinning(st));
    tm.lap("sw best hit: wait (upload, fill, walk)");
    const uint32_t *h_w = ctx->h_B.as<uint32_t>();
    return deliver_moves(ctx, batch, c, h_w, ctx->h_ta.as<uint32_t>(), h_off, 1, [](uint64_t) { return 1u; },
                         [=](uint64_t k, uint32_t) { const int32_t s = (int32_t)h_w[4 * k]; return s > 0 && s >= min_score[first + k]; }, sink, tm);
  }
  uint32_t *d_meta = ctx->t_meta.as<uint32_t>();   // head | len | score | status | pos[4]
  seqalign_trace_t t;
  memset(&t, 0, sizeof(t));
  t.str_off = ctx->t_str_off.as<uint64_t>(); t.out_a = ctx->t_out_a.as<char>(); t.out_b = ctx->t_out_b.as<char>();
  t.out_head = d_meta; t.out_len = d_meta + n; t.out_score = reinterpret_cast<int32_t *>(d_meta + 2 * n);
  t.status = d_meta + 3 * n; t.out_pos = d_meta + 4 * n; t.start_index = ctx->best_index.as<uint64_t>();
  if (dirs_used) rc = sw_traceback_dirs(ctx, sc, &d, &t, ctx->dirs.as<uint8_t>(), ctx->best_score.as<int32_t>(), st);
  else rc = seqalign_sw_traceback_device(ctx, sc, &d, &t, st);
  if (rc) return rc;
  uint32_t *h_meta = reinterpret_cast<uint32_t *>(h_off + n);
  HIP_TRY(hipMemcpyAsync(h_meta, d_meta, n * 32, hipMemcpyDeviceToHost, st));
  if ((rc = fetch_status(ctx, c, nullptr))) return rc;   // syncs
  return deliver_strings(ctx, st, n, h_meta, d_meta, ctx->t_str_off.as<uint64_t>(), [=](uint64_t w) { return first + w; },
                         [=](uint64_t w, int32_t score) { return score > 0 && score >= min_score[first + w]; }, sink, tm);
}

}  // namespace

// every pair through the host: matrices and compacted candidates copied back, hits enumerated by host threads
static int sw_batch_host_enumeration(seqalign_ctx *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                     const seqalign_dev_scoring *sc, const int32_t *min_score, uint32_t max_hits,
                                     HitSink &sink, uint64_t *n_hits) {
  int rc = SEQALIGN_OK;
  const size_t budget = std::min<size_t>(ctx->chunk_budget, (size_t)6 << 30);

  // the reduction kernel takes one threshold per launch: group by threshold
  // inside a chunk (the CLI default depends only on the lengths, so batches of
  // equal-length pairs need a single launch)
  for (const Chunk &c : plan_chunks(batch, budget)) {
    // sources / targets of asynchronous copies: declared before the guard, so that they outlive its
    // hipStreamSynchronize on every way out of this iteration
    std::vector<uint64_t> c_off;
    std::vector<uint32_t> c_cap, h_cidx;
    std::vector<int32_t> h_cscore;
    StreamSyncOnExit chunk_sync(ctx->stream);
    seqalign_dev_batch_t d;
    if ((rc = run_chunk(ctx, batch, c, sc, &d))) break;
    const uint64_t n = c.count;
    int32_t thr = min_score[c.first];
    for (uint64_t k = 1; k < n; ++k) thr = std::min(thr, min_score[c.first + k]);

    // pass 1: counts (capacity 0), pass 2: compaction
    if ((rc = ctx->best_score.reserve(n * 4)) || (rc = ctx->best_index.reserve(n * 8)) ||
        (rc = ctx->cand_count.reserve(n * 4)) || (rc = ctx->cand_off.reserve(n * 8)) ||
        (rc = ctx->cand_cap.reserve(n * 4)))
      break;
    seqalign_sw_reduce_t r;
    memset(&r, 0, sizeof(r));
    r.n_pairs = n; r.len_a = d.len_a; r.len_b = d.len_b; r.mat_off = d.mat_off; r.match_scores = d.match_scores;
    r.min_score = thr; r.best_score = ctx->best_score.as<int32_t>(); r.best_index = ctx->best_index.as<uint64_t>();
    r.cand_count = ctx->cand_count.as<uint32_t>();
    if ((rc = seqalign_sw_reduce_device(ctx, &r, ctx->stream))) break;
    if ((rc = ctx->h_misc.reserve(n * (4 + 8 + 4)))) break;
    uint32_t *h_count = ctx->h_misc.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(h_count, ctx->cand_count.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(stream_wait_spinning(ctx->stream));
    c_off.resize(n);
    c_cap.assign(h_count, h_count + n);
    uint64_t total = 0;
    for (uint64_t k = 0; k < n; ++k) { c_off[k] = total; total += c_cap[k]; }
    if ((rc = ctx->cand_index.reserve(total * 4 + 4)) || (rc = ctx->cand_score.reserve(total * 4 + 4))) break;
    HIP_TRY(hipMemcpyAsync(ctx->cand_off.p, c_off.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->cand_cap.p, c_cap.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    r.cand_off = ctx->cand_off.as<uint64_t>(); r.cand_cap = ctx->cand_cap.as<uint32_t>();
    r.cand_index = ctx->cand_index.as<uint32_t>(); r.cand_score = ctx->cand_score.as<int32_t>();
    if ((rc = seqalign_sw_reduce_device(ctx, &r, ctx->stream))) break;

    const size_t bytes = c.cells * 4;
    if ((rc = ctx->h_M.reserve(bytes)) || (rc = ctx->h_A.reserve(bytes)) || (rc = ctx->h_B.reserve(bytes))) break;
    h_cidx.resize(total + 1);
    h_cscore.resize(total + 1);
    hipError_t e = hipMemcpyAsync(ctx->h_M.p, ctx->M.p, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_A.p, ctx->A.p, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_B.p, ctx->B.p, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && total) e = hipMemcpyAsync(h_cidx.data(), ctx->cand_index.p, total * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && total) e = hipMemcpyAsync(h_cscore.data(), ctx->cand_score.p, total * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) { rc = fail_hip(e, "D2H SW results"); break; }
    if ((rc = fetch_status(ctx, c, nullptr))) break;

    // host: hit enumeration with a fresh visited mask per pair (reference
    // smith_waterman.c:165-277 semantics).  Pairs are independent -> host threads.
    std::vector<uint64_t> cell0(n);
    { uint64_t cell = 0;
      for (uint64_t k = 0; k < n; ++k) {
        cell0[k] = cell;
        cell += (uint64_t)(batch->len_a[c.first + k] + 1ull) * (batch->len_b[c.first + k] + 1ull);
      } }
    std::vector<PairHits> per_pair(n);
    std::atomic<int> first_error{SEQALIGN_OK};
    parallel_for(n, [&](uint64_t k) {
      const uint64_t p = c.first + k;
      sa_view_t v;
      v.sc = scoring; v.a = batch->arena + batch->off_a[p]; v.b = batch->arena + batch->off_b[p];
      v.len_a = batch->len_a[p]; v.len_b = batch->len_b[p];
      v.M = ctx->h_M.as<int32_t>() + cell0[k]; v.A = ctx->h_A.as<int32_t>() + cell0[k];
      v.B = ctx->h_B.as<int32_t>() + cell0[k];
      std::vector<Cand> cand;
      cand.reserve(c_cap[k]);
      for (uint32_t q = 0; q < c_cap[k]; ++q) {
        const Cand cd{h_cidx[c_off[k] + q], h_cscore[c_off[k] + q]};
        if (cd.score >= min_score[p]) cand.push_back(cd);
      }
      int prc = enumerate_hits(v, cand, max_hits, per_pair[k]);
      if (prc != SEQALIGN_OK) { int expected = SEQALIGN_OK; first_error.compare_exchange_strong(expected, prc); }
    });
    if ((rc = first_error.load())) break;
    for (uint64_t k = 0; k < n && rc == SEQALIGN_OK; ++k) {
      const PairHits &ph = per_pair[k];
      for (size_t i = 0; i < ph.hits.size(); ++i) {
        seqalign_sw_hit_t h = ph.hits[i];
        const uint64_t at = h.str_off;
        h.pair = c.first + k;
        if (!sink.put(ctx, h, ph.str_a.data() + at, ph.str_b.data() + at)) { rc = SEQALIGN_E_NOMEM; break; }
      }
    }
    if (rc) break;
  }
  *n_hits = sink.found;
  return rc;
}

static int sw_batch_impl(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                         const int32_t *min_score, uint32_t max_hits, seqalign_sw_hit_t *hits,
                         uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b, uint64_t str_cap) {
  *n_hits = 0;
  int rc = check_batch(batch);
  if (rc) return rc;
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, 1, &sc))) return rc;
  if ((rc = admit_batch(sc, batch, SA_FRAMES_FILL))) return rc;
  HitSink sink{hits, hit_cap, out_a, out_b, str_cap};
  if (max_hits == 0) return SEQALIGN_OK;
  if (max_hits == 1 && !traceback_on_host(ctx)) {   // best hit only: nothing but the strings crosses PCIe
    for (const Chunk &c : plan_chunks(batch, ctx->chunk_budget))
      if ((rc = sw_chunk_best_hit(ctx, batch, c, sc, min_score, sink))) {
        if (rc == SEQALIGN_E_NOMEM) *n_hits = sink.found;   // (out of the caller's room: what fitted is delivered; any other error: nothing is)
        return rc;
      }
    *n_hits = sink.found;
    return SEQALIGN_OK;
  }
  uint32_t max_a = 0, max_b = 0;
  for (uint64_t p = 0; p < batch->n_pairs; ++p) { max_a = std::max(max_a, batch->len_a[p]); max_b = std::max(max_b, batch->len_b[p]); }
  // (a key that does not fit the sweep's records -- scores beyond 2^28 on sequences beyond 2^16 -- goes to the host)
  if (!traceback_on_host(ctx) && key_layout_fits(key_layout(sc, max_a, max_b))) {
    // a chunk holds its pairs' three matrices + each pair's OWN part of the scratch arena (rows' candidate columns, hits'
    // keys: a pair with a low min_score needs more of it than the batch's average, so it is counted per pair)
    std::vector<uint64_t> extra(batch->n_pairs);
    { const int64_t best = best_move(sc);
      for (uint64_t p = 0; p < batch->n_pairs; ++p)
        extra[p] = 8 * hit_arena_elements(batch->len_a[p], batch->len_b[p], min_score[p], best) + 64;
    }
    for (const Chunk &c : plan_chunks(batch, ctx->chunk_budget, 12, extra.data())) {
      if ((rc = sw_chunk_device_enumerate(ctx, batch, c, sc, min_score, max_hits, sink))) break;
    }
    *n_hits = sink.found;
    return rc;
  }
  return sw_batch_host_enumeration(ctx, batch, scoring, sc, min_score, max_hits, sink, n_hits);
}

extern "C" int seqalign_sw_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                 const int32_t *min_score, uint32_t max_hits, seqalign_sw_hit_t *hits,
                                 uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b, uint64_t str_cap) {
  if (!ctx || !scoring || !min_score || !hits || !n_hits || !out_a || !out_b) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return sw_batch_impl(ctx, batch, scoring, min_score, max_hits, hits, hit_cap, n_hits, out_a, out_b, str_cap);
}

// Local hits as CIGAR (include/seqalign_hip.h): the same call with one text per hit instead of two.  On the direction-byte paths
// (the one-trip multi-hit call, the packed best-hit call) the walks come home as bit planes and the CIGAR is run-length encoded
// from those, its exact length counted first so that the hits still lie back to back in `cigar`; the paths whose walkers write
// strings (three matrices, the host enumeration) encode those strings (put_alignment).
extern "C" int seqalign_sw_batch_cigar(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                       const int32_t *min_score, uint32_t max_hits, int format, seqalign_sw_hit_t *hits,
                                       uint64_t hit_cap, uint64_t *n_hits, char *cigar, uint64_t cigar_cap) {
  if (!ctx || !scoring || !min_score || !hits || !n_hits || !cigar || (format != SEQALIGN_CIGAR_M && format != SEQALIGN_CIGAR_EQX))
    return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  CigarScope mode(ctx, format, !scoring->case_sensitive);
  return sw_batch_impl(ctx, batch, scoring, min_score, max_hits, hits, hit_cap, n_hits, cigar, cigar, cigar_cap);
}
