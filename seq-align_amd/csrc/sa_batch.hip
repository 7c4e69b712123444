// sa_batch.hip -- host-level entry points over HOST batches: chunking, packing, the fill with the
// matrices copied back (seqalign_fill_batch) and global alignment (seqalign_nw_batch).
#include <optional>

#include "sa_ctx.hpp"

using namespace sa_host;


// ------------------------------------------------- host-level: chunked fill ---

// cut the batch into chunks whose matrices (12 B/cell, plus whatever else the caller keeps per cell) fit the budget
std::vector<Chunk> sa_host::plan_chunks(const seqalign_batch_t *b, size_t budget, size_t bytes_per_cell, const uint64_t *extra_bytes) {
  std::vector<Chunk> out;
  Chunk c;
  const uint64_t per_cell = std::max<size_t>(bytes_per_cell, 1);
  uint64_t used = 0;   // device bytes of the chunk being built: its cells + what each of its pairs needs besides (extra_bytes[p])
  for (uint64_t p = 0; p < b->n_pairs; ++p) {
    const uint64_t cells = (uint64_t)(b->len_a[p] + 1ull) * (b->len_b[p] + 1ull);
    const uint64_t need = cells * per_cell + (extra_bytes ? extra_bytes[p] : 0);
    if (c.count && used + need > budget) { out.push_back(c); c = Chunk(); c.first = p; used = 0; }
    used += need;
    c.count++; c.cells += cells; c.seq_bytes += (uint64_t)b->len_a[p] + b->len_b[p];
    c.max_a = std::max(c.max_a, b->len_a[p]); c.max_b = std::max(c.max_b, b->len_b[p]);
  }
  if (c.count) out.push_back(c);
  return out;
}

// The context's auxiliary streams: [0] uploads, [1] downloads, [2] walks beside fills.  What they are for is running
// BESIDE the kernels of ctx->stream, and that takes separate hardware queues: the runtime multiplexes all streams of one
// priority over four of them, assigned as streams are first used -- a process that has used another stream or two of its
// own before the first host-level call (bench.py: a torch stream for the fills) gets the walk stream on the fills' queue,
// and the pipeline runs fill, walk and download one after the other (rocprofv3 timeline, C5's share: 7.2 instead of 5.8
// ms).  Streams of another PRIORITY come from another pool of queues, so uploads are a low-priority stream and downloads
// and walks high-priority ones, whatever the application has created at the default priority.
int sa_host::ensure_copy_streams(seqalign_ctx *ctx, int count) {
  int least = 0, greatest = 0;
  bool have_range = false;
  for (int k = 0; k < count; ++k) {
    if (ctx->copy_streams[k]) continue;
    if (!have_range) { HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest)); have_range = true; }
    HIP_TRY(hipStreamCreateWithPriority(&ctx->copy_streams[k], hipStreamNonBlocking, k == 0 ? least : greatest));
  }
  return SEQALIGN_OK;
}

// Upload one chunk (sequences packed back to back, matrices packed in pair
// order) and run the fill.  On return the device buffers of ctx hold the
// results; the stream is NOT synchronised.
// best_done (optional): ask the fill for the SW best cell per pair (into ctx->best_score / best_index);
// *best_done tells whether the fill kernel delivered it.
namespace {
// SURVEY 8e's "bucket by shape" for the packed two-pairs-per-wave fills: which of the pairs [k0, k1) go two per wave (consecutive
// list entries 2u, 2u + 1 have the same shape) and which alone.  A direct-mapped table over (len_a, len_b) holds the one pair of each
// shape that is still waiting for a partner -- one pass pairs the pairs up, a second collects who is left -- so a chunk of reads of
// every length between 100 and 150 (2 601 shapes, ~6 pairs of each per sub-batch) runs ~5/6 of its pairs through the packed kernel
// where round 3's majority vote found no majority at all.  out: the paired entries, then the pairs left over, once each (the NW
// fill's mixed grid) or as (k, k) (`alone_twice`: the SW fills, a wave to itself); returns where the paired entries end.  One table
// per host thread, kept: (max_a + 1) (max_b + 1) <= kShapeTableMax entries, 4 MiB at most.
uint32_t pair_up_shapes(const uint32_t *len_a, const uint32_t *len_b, uint64_t k0, uint64_t k1, uint32_t max_a, uint32_t max_b,
                        uint32_t *out, bool alone_twice) {
  static thread_local std::vector<uint32_t> table;
  const uint64_t Wb = (uint64_t)max_b + 1, entries = ((uint64_t)max_a + 1) * Wb;
  if (table.size() < entries) table.resize(entries);
  for (uint64_t k = k0; k < k1; ++k) table[(uint64_t)len_a[k] * Wb + len_b[k]] = ~0u;   // (only the shapes that occur are reset)
  uint32_t at = 0;
  for (uint64_t k = k0; k < k1; ++k) {
    uint32_t &slot = table[(uint64_t)len_a[k] * Wb + len_b[k]];
    if (slot == ~0u) { slot = (uint32_t)k; continue; }
    out[at++] = slot; out[at++] = (uint32_t)k;
    slot = ~0u;
  }
  const uint32_t paired_end = at;
  for (uint64_t k = k0; k < k1; ++k) {
    uint32_t &slot = table[(uint64_t)len_a[k] * Wb + len_b[k]];
    if (slot != (uint32_t)k) continue;
    out[at++] = (uint32_t)k;
    if (alone_twice) out[at++] = (uint32_t)k;
    slot = ~0u;
  }
  return paired_end;
}

// The descriptors of pairs [ka, kz) of a chunk that starts at pair `first` of the batch: sequences (and string slots) back to back
// from character `pos`, cells from `cell`, cells_of(la, lb) of them per pair -- whatever the chunk's layout gives a pair.  Returns
// where the cells end.
template <class CellsOf>
uint64_t place_pairs(const seqalign_batch_t *b, uint64_t first, const DescBlock &h, uint64_t ka, uint64_t kz, uint64_t pos, uint64_t cell,
                     CellsOf cells_of) {
  for (uint64_t k = ka; k < kz; ++k) {
    const uint32_t la = b->len_a[first + k], lb = b->len_b[first + k];
    if (h.slot) h.slot[k] = pos;               // a pair's string slot is len_a + len_b chars: the same prefix as the sequences'
    h.off_a[k] = pos; pos += la; h.off_b[k] = pos; pos += lb;
    h.len_a[k] = la; h.len_b[k] = lb;
    h.mat_off[k] = cell; cell += cells_of(la, lb);
  }
  return cell;
}

// ... and their sequences into the packed arena at those offsets: one copy where the caller's arena already has them back to back
// (`packed`: BlkSum::packed, any batch built pair by pair), else pair by pair
void pack_pairs(const seqalign_batch_t *b, uint64_t first, const DescBlock &h, uint8_t *h_seq, uint64_t ka, uint64_t kz, bool packed) {
  if (kz <= ka) return;
  if (packed) {
    memcpy(h_seq + h.off_a[ka], b->arena + b->off_a[first + ka], h.off_b[kz - 1] + h.len_b[kz - 1] - h.off_a[ka]);
    return;
  }
  for (uint64_t k = ka; k < kz; ++k) {
    memcpy(h_seq + h.off_a[k], b->arena + b->off_a[first + k], h.len_a[k]);
    memcpy(h_seq + h.off_b[k], b->arena + b->off_b[first + k], h.len_b[k]);
  }
}
// pairs [k0, k1) by the thread pool, `task` pairs per task
void pack_range(const seqalign_batch_t *b, uint64_t first, const DescBlock &h, uint8_t *h_seq, uint64_t k0, uint64_t k1, uint64_t task) {
  parallel_for((k1 - k0 + task - 1) / task, [=](uint64_t t) { pack_pairs(b, first, h, h_seq, k0 + t * task, std::min(k1, k0 + (t + 1) * task), false); });
}
}  // namespace

int sa_host::run_chunk(seqalign_ctx *ctx, const seqalign_batch_t *b, const Chunk &c,
                       const seqalign_dev_scoring *sc, seqalign_dev_batch_t *dev_out, bool *best_done,
                       const SaCandBox *cand, bool *cand_done, uint64_t uniform_stride) {
  // uniform_stride != 0 (the caller checked that every pair of the chunk has the same shape): pair k's cells start at
  // k * uniform_stride instead of back to back (the packed fills' layout, sa_fill_dirs_x2.hip).
  // uniform_stride == kBucketShapes (the caller checked that the packed fill takes the chunk's largest shape): a RAGGED chunk
  // for the packed fills -- every pair's cells start on a multiple of 256, and the chunk comes with a list that pairs up its
  // pairs of equal shape (pair_up_shapes; a pair without a partner has a wave to itself)
  const bool bucket = uniform_stride == kBucketShapes;
  if (bucket) uniform_stride = 0;
  const uint64_t n = c.count;
  int rc;
  StageTimer tm(ctx->opt.timing);
  const size_t desc_bytes = DescBlock::bytes(n, false, bucket);   // (pinned; the device copy travels as the one block it is on the host)
  if ((rc = ctx->h_desc.reserve(desc_bytes))) return rc;
  if ((rc = ctx->h_arena.reserve(c.seq_bytes + 16))) return rc;
  const DescBlock h(ctx->h_desc.p, n, false);
  uint8_t *h_seq = ctx->h_arena.as<uint8_t>();
  const bool no_matrices = cand && cand->best_only;   // direction bytes + the best cell only (the caller's cand->dirs)
  // (the best-hit fill's direction bytes -- nobody's but the walkers' -- in blocks of 8 x 16 cells: sa_kernels.h)
  const bool blocked = no_matrices && sa_dirs_blocked_shape(c.max_a);
  const uint64_t mat_total = place_pairs(b, c.first, h, 0, n, 0, 0, [=](uint32_t la, uint32_t lb) -> uint64_t {   // offsets: a sequential prefix
    return uniform_stride ? uniform_stride : bucket ? dirs_bytes256(blocked, la, lb)
         : blocked ? sa_dirs_blocked_bytes(la, lb) : (uint64_t)(la + 1ull) * (lb + 1ull);
  });
  if ((rc = ctx->arena.reserve(c.seq_bytes + 16))) return rc;
  if ((rc = ctx->off_a.reserve(desc_bytes)) || (rc = ctx->status.reserve(n * 8))) return rc;
  // (a caller that laid the chunk out for the packed direction-byte fill has reserved unplaced arenas: sa_batch_sw.hip -- asking for
  // placed ones here would replace the set it already points into)
  const bool packed_dirs = cand && cand->dirs && (bucket || uniform_stride);
  if (!no_matrices && (rc = reserve_arenas(ctx, mat_total * 4, !packed_dirs))) return rc;
  hipStream_t st = ctx->stream;
  // (bucket) entries of the chunk's pair list: the paired ones, then (k, k) for every pair left over
  const uint32_t list_len = bucket ? 2 * (uint32_t)n - pair_up_shapes(h.len_a, h.len_b, 0, n, c.max_a, c.max_b, h.list, true) : 0;
  HIP_TRY(hipMemcpyAsync(ctx->off_a.p, h.off_a, desc_bytes, hipMemcpyHostToDevice, st));
  const DescBlock dv(ctx->off_a.p, n, false);
  if (best_done && ((rc = ctx->best_score.reserve(n * 4)) || (rc = ctx->best_index.reserve(n * 8)))) return rc;
  auto range_desc = [&](uint64_t k0, uint64_t k1) {
    seqalign_dev_batch_t d = dv.range(k0, k1, ctx->arena.as<uint8_t>(), ctx->M.as<int32_t>(), ctx->A.as<int32_t>(), ctx->B.as<int32_t>(),
                                      ctx->status.as<uint64_t>(), c.max_a, c.max_b);
    if (no_matrices) d.match_scores = d.gap_a_scores = d.gap_b_scores = nullptr;
    return d;
  };
  // the fill of pairs [k0, k1) of the chunk (the whole chunk: 0, n -- always, for a ragged chunk with its list) with whatever the
  // caller asked the fill to report: nothing, the best cell, the best cell beside direction bytes only, the candidates' boxes
  auto fill_range = [&](uint64_t k0, uint64_t k1, bool *bd, bool *cd, bool *du) -> int {
    const seqalign_dev_batch_t d = range_desc(k0, k1);
    int32_t *best_score = best_done ? ctx->best_score.as<int32_t>() + k0 : nullptr;
    uint64_t *best_index = best_done ? ctx->best_index.as<uint64_t>() + k0 : nullptr;
    if (!cand)
      return best_done ? fill_device(ctx, sc, &d, SEQALIGN_KERNEL_AUTO, st, best_score, best_index, bd)
                       : seqalign_fill_batch_device(ctx, sc, &d, SEQALIGN_KERNEL_AUTO, st);
    SaCandBox sub = *cand;
    bool used = false;
    sub.uniform_stride = bucket ? 256 : uniform_stride;
    sub.dirs_used = (bucket || no_matrices || cand->dirs_used) ? &used : nullptr;
    if (bucket) { sub.pair_list = dv.list; sub.list_count = list_len; }   // (entries index the CHUNK's arrays)
    // per-pair arrays move with the range; hit_off holds absolute offsets into the scratch arena
    if (!no_matrices) { sub.cand_count += k0; sub.cand_box += 4 * k0; sub.cand_min += k0; sub.hit_off += k0; }
    const int r = no_matrices ? fill_device(ctx, sc, &d, SEQALIGN_KERNEL_AUTO, st, best_score, best_index, bd, &sub, nullptr)
                              : fill_device(ctx, sc, &d, SEQALIGN_KERNEL_AUTO, st, nullptr, nullptr, nullptr, &sub, cd);
    if (du) *du = used;
    if (!r && bucket && !used) { set_last_error("internal error: the packed fill refused a ragged chunk it had accepted"); return SEQALIGN_E_HIP; }
    return r;
  };
  // The sequences: packed by the thread pool 256 pairs per task, uploaded in slices of at least 2 048 pairs on the context's upload stream;
  // with many pairs the fill is launched slice by slice behind them (the first quarter of the pairs is being filled
  // while the rest is still being packed and shipped: C3's 11.5 MB of sequences cost 0.35 ms before the fill could
  // start), otherwise once, behind the last slice.
  constexpr uint64_t kPack = 2048;
  // (the packed two-pairs-per-wave fills take the chunk in ONE launch behind the whole upload: a first slice of 2 048 pairs to
  // start on while the rest is shipped made C3 4.31-4.34 ms where one launch makes 4.22-4.28 -- half as many waves per launch
  // leave the chip half empty for the length of a pair, and slices of a quarter of C3's 10 000 pairs are 1 000-2 000 waves on a
  // chip with 8 192 wave slots, one after the other: 1.06 + 1.44 ms where one launch takes 2.15; option subbatches = 1: one launch
  // for the other fills too)
  const uint64_t n_sub = (n >= 8192 && c.seq_bytes >= ((uint64_t)4 << 20) && ctx->opt.subbatches != 1 && !uniform_stride && !bucket) ? 4 : 1;
  // (one launch: the upload still goes in slices, packing slice i + 1 beside the copy of slice i -- 2 MiB each, so that the copy
  // engine starts after ~20 us of packing and never waits for the host: C3's 11.5 MB 0.33 -> 0.28 ms)
  const uint64_t slice_bytes = n_sub > 1 ? (c.seq_bytes + n_sub - 1) / n_sub : ((uint64_t)2 << 20);
  { int rc_s = ensure_copy_streams(ctx, 1); if (rc_s) return rc_s; }
  hipStream_t su = ctx->copy_streams[0];
  StreamSyncOnExit sync_u(su);
  EventList ev;
  HIP_TRY(ev.add(hipEventDisableTiming));
  HIP_TRY(hipEventRecord(ev.ev[0], st));          // the descriptors are on their way on st: uploads go after them
  HIP_TRY(hipStreamWaitEvent(su, ev.ev[0], 0));
  bool first = true, consistent = true, bd0 = false, cd0 = false, du0 = false;
  uint64_t filled_to = 0;
  for (uint64_t k0 = 0; k0 < n;) {
    uint64_t k1 = k0;
    while (k1 < n && (k1 == k0 || h.off_a[k1] - h.off_a[k0] < slice_bytes)) k1 = std::min(n, k1 + kPack);
    if (n - k1 < kPack) k1 = n;   // no crumb at the end
    // (tasks of 256 pairs: C4's 4 000 pairs in tasks of 2 048 kept two threads busy and fourteen idle)
    pack_range(b, c.first, h, h_seq, k0, k1, 256);
    const uint64_t lo = h.off_a[k0], hi = k1 < n ? h.off_a[k1] : c.seq_bytes;
    if (hi > lo) HIP_TRY(hipMemcpyAsync(ctx->arena.as<uint8_t>() + lo, h_seq + lo, hi - lo, hipMemcpyHostToDevice, su));
    HIP_TRY(ev.add(hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev.ev.back(), su));
    HIP_TRY(hipStreamWaitEvent(st, ev.ev.back(), 0));
    if (n_sub > 1 && consistent) {
      bool bd = false, cd = false, du = false;
      if ((rc = fill_range(k0, k1, &bd, &cd, &du))) return rc;
      if (first) { bd0 = bd; cd0 = cd; du0 = du; first = false; }
      else if (bd != bd0 || cd != cd0 || du != du0) consistent = false;   // (cannot happen with >= 2 048 pairs per slice; see below)
      filled_to = k1;
    }
    k0 = k1;
  }
  tm.lap("run_chunk: pack + H2D");
  const seqalign_dev_batch_t d = range_desc(0, n);
  if (n_sub > 1 && consistent && filled_to == n) {
    if (best_done) *best_done = bd0;
    if (cand_done) *cand_done = cd0;
    if (cand && cand->dirs_used) *cand->dirs_used = du0;
    rc = SEQALIGN_OK;
  } else {
    // one launch over the whole chunk (also the way out if the slices' fills had chosen differently: a refill is
    // idempotent)
    bool bd = false, cd = false, du = false;
    rc = fill_range(0, n, &bd, &cd, &du);
    if (best_done) *best_done = bd;
    if (cand_done) *cand_done = cd;
    if (cand && cand->dirs_used) *cand->dirs_used = du;
  }
  if (rc) return rc;
  tm.lap("run_chunk: enqueue fill");
  if (dev_out) *dev_out = d;
  return SEQALIGN_OK;
}

// fetch the per-pair status words; returns UNKNOWN_PAIR if any pair flagged
int sa_host::fetch_status(seqalign_ctx *ctx, const Chunk &c, uint64_t *status_out) {
  int rc;
  if ((rc = ctx->h_misc.reserve(c.count * 8))) return rc;
  uint64_t *h = ctx->h_misc.as<uint64_t>();
  HIP_TRY(hipMemcpyAsync(h, ctx->status.p, c.count * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(stream_wait_spinning(ctx->stream));
  rc = SEQALIGN_OK;
  for (uint64_t k = 0; k < c.count; ++k) {
    if (status_out) status_out[c.first + k] = h[k];
    if (h[k] != ~0ull) rc = SEQALIGN_E_UNKNOWN_PAIR;
  }
  return rc;
}

int sa_host::check_batch(const seqalign_batch_t *b) {
  if (!batch_readable(b)) return SEQALIGN_E_ARG;
  for (uint64_t p = 0; p < b->n_pairs; ++p)
    if ((uint64_t)(b->len_a[p] + 1ull) * (b->len_b[p] + 1ull) >= (1ull << 31)) return SEQALIGN_E_TOO_LARGE;
  return SEQALIGN_OK;
}


// Device -> pageable host memory.  A plain hipMemcpy to pageable memory is staged
// by the runtime at ~12 GB/s; large copies go through our own two pinned buffers
// instead: the DMA of slice i+1 overlaps a multi-threaded memcpy of slice i into
// the caller's buffer.  The stream must be idle w.r.t. `src` producers (it is
// enqueued behind them) and is synchronised on return.
static int copy_out_pipelined(seqalign_ctx *ctx, void *dst, const void *src_dev, size_t bytes) {
  const size_t kSlice = (size_t)32 << 20;
  if (bytes < (size_t)4 << 20) {
    HIP_TRY(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SEQALIGN_OK;
  }
  int rc;
  if ((rc = ctx->h_M.reserve(kSlice)) || (rc = ctx->h_A.reserve(kSlice))) return rc;
  void *pin[2] = {ctx->h_M.p, ctx->h_A.p};
  EventList events;   // destroyed on every exit path
  HIP_TRY(events.add(hipEventDisableTiming));
  HIP_TRY(events.add(hipEventDisableTiming));
  const hipEvent_t *ev = events.ev.data();
  StreamSyncOnExit sync(ctx->stream);   // the pinned slices are read by host threads: never leave with a DMA in flight
  const size_t n_slices = (bytes + kSlice - 1) / kSlice;
  hipError_t e = hipSuccess;
  for (size_t i = 0; i <= n_slices && e == hipSuccess; ++i) {
    if (i < n_slices) {
      const size_t off = i * kSlice, len = std::min(kSlice, bytes - off);
      e = hipMemcpyAsync(pin[i & 1], static_cast<const char *>(src_dev) + off, len, hipMemcpyDeviceToHost, ctx->stream);
      if (e == hipSuccess) e = hipEventRecord(ev[i & 1], ctx->stream);
    }
    if (i > 0 && e == hipSuccess) {
      const size_t j = i - 1, off = j * kSlice, len = std::min(kSlice, bytes - off);
      e = hipEventSynchronize(ev[j & 1]);
      if (e == hipSuccess) parallel_memcpy(static_cast<char *>(dst) + off, pin[j & 1], len);
    }
  }
  if (e != hipSuccess) return fail_hip(e, "pipelined D2H");
  return SEQALIGN_OK;
}

extern "C" int seqalign_fill_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                   int is_sw, const uint64_t *mat_off, int32_t *M, int32_t *A, int32_t *B,
                                   uint64_t *status) {
  if (!ctx || !scoring || !mat_off || !M || !A || !B) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  int rc = check_batch(batch);
  if (rc) return rc;
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, is_sw, &sc))) return rc;
  if ((rc = admit_batch(sc, batch, SA_FRAMES_FILL))) return rc;
  return fill_batch_uploaded(ctx, batch, sc, mat_off, M, A, B, status);
}

int sa_host::fill_batch_uploaded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const seqalign_dev_scoring *sc,
                                 const uint64_t *mat_off, int32_t *M, int32_t *A, int32_t *B, uint64_t *status) {
  int rc = SEQALIGN_OK;
  int worst = SEQALIGN_OK;
  for (const Chunk &c : plan_chunks(batch, ctx->chunk_budget)) {
    if ((rc = run_chunk(ctx, batch, c, sc, nullptr))) break;
    // Small chunks -- the legacy one-pair-per-call API above all -- in ONE round trip: the three matrices and the status
    // words into pinned staging behind each other, one synchronisation, then plain memcpys.  (One pair used to cost
    // four: three pageable copies, each waited for, and the status.)
    const size_t small = c.cells * 4;
    if (3 * small <= ((size_t)4 << 20)) {
      const size_t status_at = (3 * small + 7) & ~(size_t)7;   // (uint64 words: 8-byte aligned whatever the cell count)
      if ((rc = ctx->h_M.reserve(status_at + c.count * 8 + 64))) break;
      char *pin = ctx->h_M.as<char>();
      hipStream_t st = ctx->stream;
      StreamSyncOnExit sync(st);
      HIP_TRY(hipMemcpyAsync(pin, ctx->M.p, small, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(pin + small, ctx->A.p, small, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(pin + 2 * small, ctx->B.p, small, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(pin + status_at, ctx->status.p, c.count * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      uint64_t dev_cell = 0;
      const uint64_t *h_status = reinterpret_cast<const uint64_t *>(pin + status_at);
      for (uint64_t k = 0; k < c.count; ++k) {
        const uint64_t p = c.first + k, cells = (uint64_t)(batch->len_a[p] + 1ull) * (batch->len_b[p] + 1ull);
        memcpy(M + mat_off[p], pin + dev_cell * 4, cells * 4);
        memcpy(A + mat_off[p], pin + small + dev_cell * 4, cells * 4);
        memcpy(B + mat_off[p], pin + 2 * small + dev_cell * 4, cells * 4);
        dev_cell += cells;
        if (status) status[p] = h_status[k];
        if (h_status[k] != ~0ull) worst = SEQALIGN_E_UNKNOWN_PAIR;
      }
      continue;
    }
    // copy back: runs of pairs that are contiguous in the caller's arenas go in one piece
    uint64_t k = 0, dev_cell = 0;
    while (k < c.count) {
      uint64_t run_cells = 0, j = k;
      const uint64_t host0 = mat_off[c.first + k];
      while (j < c.count && mat_off[c.first + j] == host0 + run_cells) {
        run_cells += (uint64_t)(batch->len_a[c.first + j] + 1ull) * (batch->len_b[c.first + j] + 1ull);
        ++j;
      }
      const size_t bytes = run_cells * 4;
      if ((rc = copy_out_pipelined(ctx, M + host0, ctx->M.as<int32_t>() + dev_cell, bytes)) ||
          (rc = copy_out_pipelined(ctx, A + host0, ctx->A.as<int32_t>() + dev_cell, bytes)) ||
          (rc = copy_out_pipelined(ctx, B + host0, ctx->B.as<int32_t>() + dev_cell, bytes)))
        break;
      dev_cell += run_cells;
      k = j;
    }
    if (rc) break;
    int src = fetch_status(ctx, c, status);   // also synchronises the stream
    if (src == SEQALIGN_E_UNKNOWN_PAIR) worst = src;
    else if (src) { rc = src; break; }
  }
  return rc ? rc : worst;
}

// ----------------------------------------------- host-level: NW over a batch ---

void sa_host::parallel_memcpy(void *dst, const void *src, size_t bytes) {
  const size_t kPiece = (size_t)2 << 20;
  const uint64_t pieces = (bytes + kPiece - 1) / kPiece;
  parallel_for(pieces, [&](uint64_t i) {
    const size_t off = i * kPiece;
    memcpy(static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, std::min(kPiece, bytes - off));
  });
}


bool sa_host::traceback_on_host(const seqalign_ctx *ctx) { return ctx->opt.traceback_host; }

// ---- seqalign_nw_batch, device traceback: one chunk as a PIPELINE of sub-batches -------------------------------
// The stages of a chunk -- host packs the sequences, H2D, fill (HBM-bound), traceback, D2H of the strings, host
// unpacks -- run strictly one after the other cost their sum (C2: 1.3-1.4 ms for a 0.41 ms fill; C5's per-GPU share:
// 12.2 ms for 5.1).  What CAN overlap, measured (profiles/r03/r03_nw_pipeline.md):
//   * the copies and the host work with the kernels: yes -- they use PCIe and the CPU;
//   * the traceback of one sub-batch with the fill of the next (two streams, the walkers at high priority): NO.
//     The walkers are not latency-bound at these sizes, they are bound by scattered 64-byte sectors (3 per step: one
//     cell of each matrix; 10 k pairs: 0.29 ms = 2 TB/s of sector traffic, 125 k pairs: 3.6 ms = the same rate), so
//     next to a fill that saturates HBM both simply slow down (walks 0.29 -> 0.5 ms per sub-batch, fills +50 %),
//     and a walk over few pairs takes its ~0.3 ms however few they are -- 16 sub-batch walks cost more than one.
// So: sub-batches of consecutive pairs for upload + fill, tracebacks over GROUPS of sub-batches (>= 32 k pairs, or
// the whole chunk) in the SAME stream as the fills, downloads and unpacking per group:
//   stream U (upload)   :  H2D(0) H2D(1) H2D(2) ...
//   stream F (kernels)  :  fill(0) fill(1) .. walk(group 0) fill(..) .. walk(group 1) ...       fill(s) waits for H2D(s)
//   stream D (download) :                        results of group 0 | group 1 ...               waits for walk(g)
//   host                :  packs every sub-batch, enqueues as it goes (the GPU starts on the first at once), then
//                          unpacks the groups in order as they land
// Same kernels, same buffers (a sub-batch is a pair range of the chunk's descriptor arrays and arenas), same results.
// With direction bytes (plain scorings, rows up to 1 024 columns: the fill writes ONE byte of directions per cell and nothing
// else, sa_fill_dirs.hip -- the three matrices are not even allocated) the fill is bound by VALU issue and a walk by the latency
// of its dependent byte loads, so there a group's walk runs on its own stream beside the next group's fills (option walk_overlap).
//
// The descriptor arrays of a chunk whose pairs all have ONE shape are arithmetic progressions: written on the device (a few
// microseconds) instead of sent over PCIe (44 B per pair: 5.5 MB for a 125 k-pair share, 0.1 ms in front of the first fill
// and 15 % on top of the sequences' bytes).  Layout of the block: DescBlock with slots (sa_ctx.hpp).
__global__ void __launch_bounds__(256) uniform_descriptors_kernel(uint64_t *desc, uint64_t n, uint32_t la, uint32_t lb, uint64_t stride) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n) return;
  uint64_t *off_a = desc, *off_b = off_a + n, *mat = off_b + n, *slot = mat + n;
  uint32_t *len_a = reinterpret_cast<uint32_t *>(slot + n + 1), *len_b = len_a + n;
  const uint64_t pos = k * ((uint64_t)la + lb);
  slot[k] = pos;
  if (k == n) return;
  off_a[k] = pos; off_b[k] = pos + la; mat[k] = k * stride; len_a[k] = la; len_b[k] = lb;
}

static uint32_t pick_subbatches(const seqalign_ctx *ctx, const Chunk &c) {
  if (ctx->opt.subbatches) return (uint32_t)std::min<uint64_t>(ctx->opt.subbatches, std::max<uint64_t>(c.count, 1));
  // by size, measured (profiles/r03/r03_nw_pipeline.md): C2 (10 k pairs) gains nothing from 2 or 4 sub-batches (1.28 ->
  // 1.34 ms: its walk must stay one launch, and two half fills are slower than one), C5's share (125 k pairs) 12.6 ->
  // 11.4 (4) -> 10.2 (8) -> 10.8 ms (16).  So: sub-batches of >= 12 288 pairs and >= 256 M cells (3 GB of matrices),
  // at most 8.
  const uint64_t by_pairs = c.count / 12288, by_cells = c.cells / (256ull << 20);
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min(by_pairs, by_cells), 8));
}

namespace {
// pairs per host task: 512 (C2: 20 tasks for 32 threads would leave a third of them idle -- but a task below ~10 us is
// all dispatch); fewer when the caller forces more sub-batches than such blocks (sub-batches are cut at block boundaries)
uint64_t host_block_pairs(const seqalign_ctx *ctx, uint64_t n) {
  uint64_t blk = 512;
  if (ctx->opt.subbatches > 1) while (blk > 1 && n / blk < 2ull * ctx->opt.subbatches) blk /= 2;
  return blk;
}
struct BlkSum {
  uint64_t chars = 0, cells = 0, cells256 = 0, blk256 = 0;   // (blk256: the pairs' direction bytes in 8 x 16 blocks, each rounded up to 256)
  uint32_t max_a = 0, max_b = 0;
  bool same = true, too_large = false;
  bool packed = true;   // the block's sequences lie in the caller's arena as they will in ours: a, b, a, b, ... back to back
};
// sizes of pairs [first, first + n) per block of kHostBlk pairs; `same`: every pair of the block has the shape of pair `first`
void scan_blocks(const seqalign_batch_t *b, uint64_t first, uint64_t n, uint64_t kHostBlk, std::vector<BlkSum> &blk) {
  const uint64_t nb = (n + kHostBlk - 1) / kHostBlk;
  blk.assign(nb, BlkSum());
  if (!n) return;
  const uint32_t la0 = b->len_a[first], lb0 = b->len_b[first];
  parallel_for(nb, [&](uint64_t bi) {
    BlkSum s;
    for (uint64_t k = bi * kHostBlk, e = std::min(n, (bi + 1) * kHostBlk); k < e; ++k) {
      const uint32_t la = b->len_a[first + k], lb = b->len_b[first + k];
      const uint64_t cells = (uint64_t)(la + 1ull) * (lb + 1ull);
      s.chars += (uint64_t)la + lb; s.cells += cells; s.cells256 += dirs_bytes256(false, la, lb);
      s.blk256 += dirs_bytes256(true, la, lb);
      s.max_a = std::max(s.max_a, la); s.max_b = std::max(s.max_b, lb);
      s.same = s.same && la == la0 && lb == lb0;
      s.too_large = s.too_large || cells >= (1ull << 31);
      s.packed = s.packed && b->off_b[first + k] == b->off_a[first + k] + la &&
                 (k + 1 == e || b->off_a[first + k + 1] == b->off_b[first + k] + lb);
    }
    blk[bi] = s;
  });
}

// ---- layout of a chunk's direction bytes: pairs back to back / every pair of ONE shape `stride` bytes apart, a multiple of 256
// (the packed fill: two or four pairs per wave in packed int16, sa_fill_dirs_x2.hip) / ragged (reads trimmed to various lengths):
// every pair on a multiple of 256, pairs of EQUAL shape are found per sub-batch (pair_up_shapes) and go two per wave, the ones
// left over one per wave, all in one grid per sub-batch (nw_dirs_fill_mixed).  blocked (round 6): rows of up to 512 columns have
// their bytes in blocks of 8 x 16 cells (sa_kernels.h) -- a pair takes ceil(rows / 8) x ceil(columns / 16) x 128 bytes and starts
// on a multiple of 256 whatever the layout of the chunk.  One rule for both result forms.
struct NwDirsLayout {
  enum Kind { kBackToBack, kUniform, kMixed } kind = kBackToBack;
  uint64_t stride = 0;
  bool blocked = false;
  uint32_t pack_a = 0, pack_b = 0;   // (kMixed) the shape the packed kernel is chosen for: the largest of the pairs that go two per wave
  uint64_t pair_bytes(uint32_t la, uint32_t lb) const {   // what one pair takes: bytes, or cells of each matrix (no direction bytes)
    return kind == kUniform ? stride : (blocked || kind == kMixed) ? dirs_bytes256(blocked, la, lb) : (uint64_t)(la + 1ull) * (lb + 1ull);
  }
  uint64_t block_bytes(const BlkSum &s, uint64_t pairs) const {   // ... and a host block of `pairs` pairs
    return kind == kUniform ? pairs * stride : blocked ? s.blk256 : kind == kMixed ? s.cells256 : s.cells;
  }
};
NwDirsLayout nw_dirs_layout(const seqalign_ctx *ctx, const seqalign_dev_scoring *sc, const Chunk &c, bool use_dirs, bool same_shape) {
  NwDirsLayout l;
  if (!use_dirs) return l;   // three matrices: cells back to back
  const uint64_t n = c.count;
  l.blocked = sa_dirs_blocked_shape(c.max_a);
  const bool may_pack = ctx->opt.pack16 && (n >= kPackedFillMinPairs || ctx->opt.pack16 == 2);
  if (same_shape && may_pack && nw_dirs_x2_applicable(ctx, sc, c.max_a, c.max_b)) {
    l.kind = NwDirsLayout::kUniform;
    l.stride = dirs_bytes256(l.blocked, c.max_a, c.max_b);
  } else if (!same_shape && may_pack && (n >= kBucketedFillMinPairs || ctx->opt.pack16 == 2) &&
             (uint64_t)(c.max_a + 1ull) * (c.max_b + 1ull) <= kShapeTableMax && nw_dirs_x2_applicable(ctx, sc, c.max_a, c.max_b)) {
    l.kind = NwDirsLayout::kMixed;
    l.pack_a = c.max_a; l.pack_b = c.max_b;
  }
  return l;
}
// Round 3's rule for a ragged chunk, kept for the STRINGS form alone: the pairs of the majority shape, if there is one, go two per
// wave and all others one per wave (Boyer-Moore vote, then an exact count: two passes of compares, no hashing).  The table rule
// above packs more pairs, but on the chunks this form was timed on it is no faster at 30 000 pairs and 0.01 to 0.02 ms slower at
// 2 600, in both orders (profiles/r31/README.md, section 5), so this form keeps its vote; the moves form, which has pipelined whole
// rounds of packed waves since round 4, keeps the table.
void majority_vote_layout(const seqalign_ctx *ctx, const seqalign_dev_scoring *sc, const seqalign_batch_t *b, const Chunk &c, NwDirsLayout &l) {
  const uint64_t n = c.count;
  l.kind = NwDirsLayout::kBackToBack;
  if (!(ctx->opt.pack16 && (n >= kBucketedFillMinPairs || ctx->opt.pack16 == 2))) return;
  auto key = [&](uint64_t k) { return (uint64_t)b->len_a[c.first + k] << 32 | b->len_b[c.first + k]; };
  uint64_t best_key = 0, votes = 0, best_count = 0;
  for (uint64_t k = 0; k < n; ++k) {
    if (votes == 0) { best_key = key(k); votes = 1; } else if (key(k) == best_key) ++votes; else --votes;
  }
  for (uint64_t k = 0; k < n; ++k) best_count += key(k) == best_key;
  const uint32_t modal_a = (uint32_t)(best_key >> 32), modal_b = (uint32_t)best_key;
  if ((best_count >= kBucketedFillMinPairs || (ctx->opt.pack16 == 2 && best_count >= 2)) && best_count * 2 >= n &&
      nw_dirs_x2_applicable(ctx, sc, modal_a, modal_b)) {
    l.kind = NwDirsLayout::kMixed;
    l.pack_a = modal_a; l.pack_b = modal_b;
  }
}
// ... and its list of pairs [k0, k1): the majority shape's pairs, then the others; returns how many of the first
uint32_t list_majority_first(const uint32_t *len_a, const uint32_t *len_b, uint64_t k0, uint64_t k1, uint32_t modal_a, uint32_t modal_b, uint32_t *out) {
  uint32_t at = 0;
  for (uint64_t k = k0; k < k1; ++k) if (len_a[k] == modal_a && len_b[k] == modal_b) out[at++] = (uint32_t)k;
  const uint32_t n_modal = at;
  for (uint64_t k = k0; k < k1; ++k) if (!(len_a[k] == modal_a && len_b[k] == modal_b)) out[at++] = (uint32_t)k;
  return n_modal;
}

// ---- the host blocks of a chunk (the moves form, seqalign_host_legs_nw): every pass over the pairs is parallel, in blocks of
// kHostBlk pairs -- sizes per block (scan_blocks), a serial prefix over the BLOCKS, then offsets + packing per block
struct HostBlocks {
  const seqalign_batch_t *batch;
  uint64_t first, n, kHostBlk;
  const std::vector<BlkSum> &blk;
  std::vector<uint64_t> chars_at, cells_at;   // where each block's pairs start: characters (sequences, string slots) and cells
  HostBlocks(const seqalign_batch_t *b, uint64_t first_, uint64_t n_, uint64_t per, const std::vector<BlkSum> &blk_, const NwDirsLayout &layout)
      : batch(b), first(first_), n(n_), kHostBlk(per), blk(blk_), chars_at(blk_.size() + 1, 0), cells_at(blk_.size() + 1, 0) {
    for (uint64_t bi = 0; bi < blk.size(); ++bi) {
      chars_at[bi + 1] = chars_at[bi] + blk[bi].chars;
      cells_at[bi + 1] = cells_at[bi] + layout.block_bytes(blk[bi], pair_at(bi + 1) - pair_at(bi));
    }
  }
  uint64_t pair_at(uint64_t bi) const { return std::min(n, bi * kHostBlk); }
  void place(const DescBlock &h, const NwDirsLayout &layout) const {   // offsets: per block from its base
    const HostBlocks *hb = this;
    parallel_for(blk.size(), [=](uint64_t bi) {
      place_pairs(hb->batch, hb->first, h, hb->pair_at(bi), hb->pair_at(bi + 1), hb->chars_at[bi], hb->cells_at[bi],
                  [&](uint32_t la, uint32_t lb) { return layout.pair_bytes(la, lb); });
    });
    h.slot[n] = chars_at.back();
  }
  // the sequences of blocks [b0, b1) into the packed arena, in quarter-block tasks (every pool thread has work in every slice)
  void pack(const DescBlock &h, uint8_t *h_seq, uint64_t b0, uint64_t b1) const {
    constexpr uint64_t kParts = 4;   // tasks per block
    const HostBlocks *hb = this;
    parallel_for((b1 - b0) * kParts, [=](uint64_t ti) {
      const uint64_t bi = b0 + ti / kParts, part = ti % kParts;
      const uint64_t kb = hb->pair_at(bi), span = hb->pair_at(bi + 1) - kb;
      pack_pairs(hb->batch, hb->first, h, h_seq, kb + span * part / kParts, kb + span * (part + 1) / kParts, hb->blk[bi].packed);
    });
  }
};

// ---- the moves of pairs [k_lo, k_hi) of a chunk, landed in pinned memory (two bit planes per pair at DescBlock::move_word, two
// words per pair: score, moves walked or SA_MOVES_ERR | code), expanded against the caller's sequences straight into the caller's
// buffers (host/sa_moves.c: vpexpandb, 64 columns per instruction) -- or, in CIGAR mode (seqalign_nw_batch_cigar), run lengths
// straight from the two planes, no strings (str_off has n + 1 entries: the slots)
struct MovesHome {
  const seqalign_batch_t *batch;
  uint64_t first;
  DescBlock h;
  const uint32_t *h_moves, *h_meta;
  int cigar_format;
  bool cigar_fold;
  const uint64_t *str_off;
  char *out_a, *out_b;
  uint32_t *out_len;
  int32_t *out_score;
};
void expand_moves(const MovesHome &home, uint64_t k_lo, uint64_t k_hi, LowestFailure &bad) {
  constexpr uint64_t kOut = 128;   // pairs per task: C2's 10 000 pairs over all 32 threads
  // (the tasks hold what they read per pair BY VALUE: DESIGN.md 3.30, 0.20 against 0.12 ms for the same loop body by reference)
  parallel_for((k_hi - k_lo + kOut - 1) / kOut, [=, &bad](uint64_t blk_i) {
    const MovesHome &m = home;
    const seqalign_batch_t *batch = m.batch;
    for (uint64_t k = k_lo + blk_i * kOut, e = std::min(k_hi, k_lo + (blk_i + 1) * kOut); k < e; ++k) {
      const uint64_t p = m.first + k;
      if (k + 6 < e) {   // the GPU wrote the moves and the words: every first touch is a miss -- have the pair six ahead on its way
        const uint64_t kn = k + 6;
        const uint32_t nwn = (m.h.len_a[kn] + m.h.len_b[kn] + 31u) >> 5;
        const uint32_t *pn = m.h_moves + m.h.move_word(kn);
        __builtin_prefetch(m.h_meta + 2 * kn); __builtin_prefetch(pn + nwn - 1); __builtin_prefetch(pn + 2 * nwn - 1);
        __builtin_prefetch(batch->arena + batch->off_a[m.first + kn]);
      }
      const uint32_t n_moves = m.h_meta[2 * k + 1];
      int prc = SEQALIGN_OK;
      if (n_moves >= SA_MOVES_ERR) {
        prc = (int)(n_moves & 15u);
      } else {
        const uint32_t la = m.h.len_a[k], lb = m.h.len_b[k], nw = (la + lb + 31u) >> 5;
        const uint32_t *pa = m.h_moves + m.h.move_word(k);
        if (m.cigar_format)
          prc = sa_cigar_nw_moves(batch->arena + batch->off_a[p], la, batch->arena + batch->off_b[p], lb, pa, pa + nw, nw, n_moves,
                                  m.cigar_format, m.cigar_fold, m.out_a + m.str_off[p], m.str_off[p + 1] - m.str_off[p], &m.out_len[p], nullptr);
        else
          prc = sa_expand_nw_moves(batch->arena + batch->off_a[p], la, batch->arena + batch->off_b[p], lb, pa, pa + nw, nw, n_moves,
                                   m.out_a + m.str_off[p], m.out_b + m.str_off[p], &m.out_len[p]);
        m.out_score[p] = (int32_t)m.h_meta[2 * k];
      }
      if (prc != SEQALIGN_OK) bad.note(k, prc);
    }
  });
}

// ---- the pipeline's plan: sub-batches, groups, streams, events
// sub-batches cut at equal cells: prefix[i] is where item i (a pair, a host block) starts, `total` where the last one ends
std::vector<uint64_t> cut_at_equal_cells(const uint64_t *prefix, uint64_t count, uint64_t total, uint32_t n_sub) {
  std::vector<uint64_t> cut(n_sub + 1, count);
  cut[0] = 0;
  uint64_t i = 0;
  for (uint32_t s = 1; s < n_sub; ++s) {
    const uint64_t want = total / n_sub * s;
    while (i < count && prefix[i] < want) ++i;
    cut[s] = std::max(i, cut[s - 1]);
  }
  return cut;
}
// ... or, for a chunk of one shape at four pairs per wave, sub-batches of whole ROUNDS of waves (4 096 pairs = 1 024 waves, one
// per SIMD) -- C5's share as 7 x 16 384 + 10 312 pairs is 31 rounds where 8 x 15 625 are 32.  In host blocks; false: not such a chunk.
bool cut_whole_rounds(uint64_t n, uint64_t nb, uint64_t kHostBlk, uint32_t n_sub, std::vector<uint64_t> &bcut) {
  if (!(n_sub > 1 && n / n_sub >= 8192 && kHostBlk <= 4096 && 4096 % kHostBlk == 0)) return false;
  const uint64_t per = (((n + n_sub - 1) / n_sub + 4095u) & ~(uint64_t)4095u) / kHostBlk;
  bcut.assign(n_sub + 1, nb);
  for (uint32_t s = 0; s < n_sub; ++s) bcut[s] = std::min<uint64_t>(nb, s * per);
  return true;
}
struct NwPipeline {
  std::vector<uint64_t> cut;     // sub-batch s = pairs [cut[s], cut[s + 1]) of the chunk
  std::vector<uint32_t> gcut;    // group g = sub-batches [gcut[g], gcut[g + 1]): filled one by one, walked and sent home together
  uint32_t n_sub, n_grp;
  bool walk_beside;              // a group's walk runs beside the next group's fills (one group: nothing to run beside)
  hipStream_t sf, su, sd, sw;    // fills (the context's stream), uploads, downloads, the walks beside (ensure_copy_streams)
  StreamSyncOnExit sync_f, sync_u, sync_d, sync_w;   // pinned / device buffers are reused by the next call: never leave work in flight
  EventList ev;                  // per sub-batch: uploaded; per group: walked, home, filled; then: descriptors up

  // (tried: a short last sub-batch as a group of its own, so that the walk + results + expansion nothing runs beside are
  // short -- C5's share 3.95 -> 4.05 ms, the extra launch and the quarter-size fill cost what the shorter tail saves)
  static std::vector<uint32_t> group_cuts(const std::vector<uint64_t> &cut) {
    constexpr uint64_t kGroupPairs = 32768;   // (measured, C5 share, walks in stream order: 2 groups 3.49 ms, 3 groups 3.31, 4 groups 3.44; round 6, tile walks: groups of 16 384 are level (C5's share 2.93-3.11 / 2.91-3.05, 65 536 pairs 1.85 / 1.70);
                                              //  with the lane walker's look-ahead 3 / 4 / 8 groups and a short last group: 3.12-3.27, no order)
    const uint32_t n_sub = (uint32_t)cut.size() - 1;
    const uint64_t n = cut[n_sub];
    std::vector<uint32_t> gcut{0};
    for (uint32_t s = 1; s < n_sub; ++s)
      if (cut[s] - cut[gcut.back()] >= kGroupPairs && n - cut[s] >= kGroupPairs / 2) gcut.push_back(s);
    gcut.push_back(n_sub);
    return gcut;
  }
  NwPipeline(seqalign_ctx *ctx, std::vector<uint64_t> pair_cuts, bool may_walk_beside)
      : cut(std::move(pair_cuts)), gcut(group_cuts(cut)), n_sub((uint32_t)cut.size() - 1), n_grp((uint32_t)gcut.size() - 1),
        walk_beside(may_walk_beside && n_grp > 1), sf(ctx->stream), su(ctx->copy_streams[0]), sd(ctx->copy_streams[1]),
        sw(walk_beside ? ctx->copy_streams[2] : sf), sync_f(sf), sync_u(su), sync_d(sd), sync_w(sw) {}
  int create_events() {
    for (uint32_t k = 0; k < n_sub + 3 * n_grp + 1; ++k) HIP_TRY(ev.add(hipEventDisableTiming));
    return SEQALIGN_OK;
  }
  hipEvent_t uploaded(uint32_t s) const { return ev.ev[s]; }                 // sub-batch s's sequences are on the device
  hipEvent_t walked(uint32_t g) const { return ev.ev[n_sub + 3 * g]; }       // group g's walk is done: its results may go home
  hipEvent_t home(uint32_t g) const { return ev.ev[n_sub + 3 * g + 1]; }     // ... and are in pinned memory
  hipEvent_t filled(uint32_t g) const { return ev.ev[n_sub + 3 * g + 2]; }   // group g's fills are done: its walk may start beside
  hipEvent_t descriptors_up() const { return ev.ev.back(); }
  // the last group's walk has no fill to run beside: it stays in the fills' stream, right behind the last fill (on its own
  // stream it waited for the previous group's download -- streams share hardware queues; rocprofv3 timeline of C5's share: 0.6 ms)
  hipStream_t walk_stream(uint32_t g) const { return g + 1 < n_grp ? sw : sf; }
};
}  // namespace

// ---- one chunk of seqalign_nw_batch on the device: plan -> enqueue -> deliver, in one of two result forms.
//
// STRINGS come home (blk == nullptr; round 3): per group the device sends back ONE block of characters (out_a | out_b of its
// pairs) and one of per-pair words (head, len, score, status interleaved: SaTraceParams::out_meta4; the fill's status is folded in
// by the walker).  It serves the three matrices, and direction bytes under option nw_moves = 0.
//
// MOVES come home (blk: scan_blocks' sums of the chunk in blocks of kHostBlk pairs; round 4, the default wherever the direction-byte
// fill takes the chunk).  What the strings form spent outside its kernels on C2 (10 k pairs, 0.89 ms per call, of which fill 0.20 +
// walk 0.12): a serial pass over the pairs for the offsets, packing on 10 of 32 threads, a descriptor copy and a sequence copy (two
// copy-engine latencies + 3 MB at 40 GB/s before the fill could start), 6 MB of gapped strings home through the runtime's blit
// kernel, unpacking on 10 threads again -- and each of the pool's dispatches paid for waking 31 sleeping threads.  Here:
//   * the fill may read the packed sequences and the descriptor arrays IN PLACE from pinned host memory (300 B per pair over
//     PCIe, hidden behind 0.2 ms of arithmetic), so the kernel is launched the moment the host has packed -- no copy, no
//     event, no second stream on the way in (option zero_copy & 1);
//   * the walk sends home two bits per alignment column instead of two characters (sa_traceback.hip: which of the two
//     strings has a gap there), written in place into pinned host memory (zero_copy & 2): C2 0.83 MB instead of 6.1 MB, no
//     blit kernel beside the next fill; the host threads expand them (expand_moves);
//   * every pass over the pairs is parallel (HostBlocks); the pool's workers stay awake between the dispatches of a call.
// A new result form supplies what the `moves` branches below do: its buffers, what the walk's SaTraceParams gets on top of
// trace_params, what goes home per group, the per-pair unpacking and its wait.
static int nw_chunk(seqalign_ctx *ctx, const seqalign_batch_t *batch, const Chunk &c, const seqalign_dev_scoring *sc,
                    const std::vector<BlkSum> *blk, uint64_t kHostBlk, const uint64_t *str_off, char *out_a, char *out_b,
                    uint32_t *out_len, int32_t *out_score) {
  const bool moves = blk != nullptr;
  const uint64_t n = c.count, total = c.seq_bytes;
  int rc;
  StageTimer tm(ctx->opt.timing);
  // in place over PCIe, measured (tools/nw_moves_bench.py, profiles/r04/r04_nw_moves_bench.txt): READING the sequences in
  // place costs more than it saves (C2 0.58 -> 0.65 ms, C5's share 3.8 -> 4.6: the fills' 64-byte reads are bound by the
  // read requests the GPU keeps in flight on the link, ~11 GB/s, where the copy engine moves 40-50); WRITING the moves in
  // place pays when the walker stores them coalesced (one wave per walk, whole words of 64 lanes: C2 0.58 -> 0.51 ms) and
  // loses when every lane stores its own 4 bytes (one lane per walk, the large groups: C5's share 3.6 -> 4.4).  So auto =
  // sequences through the copy engine, moves in place exactly when the walks run one wave each.
  const bool auto_zc = ctx->opt.zero_copy == 4u;
  // (round 6: with the direction byte's local form the tile walks are level with or ahead of the lane walkers at every batch size --
  //  30 000 pairs 0.99 / 1.04 ms, 65 536: 1.63 / 1.78, 125 000: 2.93 / 2.93-2.95 -- so they walk every chunk; dirs_local = 0: round 4's rule)
  const bool tile_walks = ctx->opt.trace_kernel ? ctx->opt.trace_kernel == 2 : (ctx->opt.dirs_local != 0 || n < SA_WALK_TILE_MAX);
  const bool zc_in = moves && !auto_zc && (ctx->opt.zero_copy & 1u) != 0;
  const bool zc_out = moves && (auto_zc ? tile_walks : (ctx->opt.zero_copy & 2u) != 0);
  // (tile walks: the fills write the direction byte's LOCAL form -- a cell's own comparisons, resolved by the walker: sa_kernels.h)
  const bool local = moves && tile_walks && ctx->opt.dirs_local;
  const bool use_dirs = moves || nw_dirs_applicable(ctx, sc, c.max_a, n);

  // ---- plan: layout, descriptors, buffers, sub-batches and groups
  bool same_shape = true;
  if (moves) for (const BlkSum &s : *blk) same_shape = same_shape && s.same;
  else for (uint64_t k = 1; k < n && same_shape; ++k) same_shape = batch->len_a[c.first + k] == batch->len_a[c.first] && batch->len_b[c.first + k] == batch->len_b[c.first];
  NwDirsLayout layout = nw_dirs_layout(ctx, sc, c, use_dirs, same_shape);
  if (!moves && use_dirs && !same_shape) majority_vote_layout(ctx, sc, batch, c, layout);
  const size_t desc_bytes = DescBlock::bytes(n, true);
  if ((rc = ctx->h_desc.reserve(desc_bytes)) || (rc = ctx->h_arena.reserve(total + 64))) return rc;
  const DescBlock h(ctx->h_desc.p, n, true);
  uint8_t *h_seq = ctx->h_arena.as<uint8_t>();
  std::optional<HostBlocks> hb;   // (moves)
  uint64_t mat_total;
  if (moves) {
    hb.emplace(batch, c.first, n, kHostBlk, *blk, layout);
    hb->place(h, layout);
    mat_total = hb->cells_at.back();
  } else {   // (one serial pass)
    mat_total = place_pairs(batch, c.first, h, 0, n, 0, 0, [&](uint32_t la, uint32_t lb) { return layout.pair_bytes(la, lb); });
    h.slot[n] = total;
  }
  // Pinned: descriptors, sequences, the results (h_ta: the moves, or the characters; h_tmeta: the per-pair words, 2 or 4); device:
  // the direction bytes and what the fill tells the walk (end score / state, status), or the three matrices -- plus staging twins
  // of the pinned blocks, except where the kernels read (zc_in) or write (zc_out) those in place
  const uint64_t move_words = 2 * ((total >> 5) + n) + 2;
  const size_t res_bytes = moves ? move_words * 4 : 2 * total + 16, meta_bytes = moves ? n * 8 : n * 16;
  if ((rc = ctx->h_ta.reserve(res_bytes)) || (rc = ctx->h_tmeta.reserve(meta_bytes)) || (rc = ctx->status.reserve(n * 8))) return rc;
  if (use_dirs) {
    if ((rc = ctx->dirs.reserve(mat_total + 4096)) || (rc = ctx->best_score.reserve(n * 4)) || (rc = ctx->best_index.reserve(n * 8))) return rc;
  } else if ((rc = reserve_arenas(ctx, c.cells * 4))) {
    return rc;
  }
  if (!zc_in && ((rc = ctx->arena.reserve(total + 64)) || (rc = ctx->off_a.reserve(desc_bytes)))) return rc;
  if (!zc_out && ((rc = ctx->t_out_a.reserve(res_bytes)) || (rc = ctx->t_meta.reserve(meta_bytes)))) return rc;
  if ((rc = ensure_copy_streams(ctx, 3))) return rc;

  // sub-batches: of pairs, cut at equal cells (strings); of host blocks, in whole rounds or cut at equal cells (moves)
  const uint64_t nb = moves ? blk->size() : 0;
  const uint32_t n_sub = moves ? (uint32_t)std::min<uint64_t>(pick_subbatches(ctx, c), nb) : pick_subbatches(ctx, c);
  std::vector<uint64_t> bcut, cut;
  if (moves) {
    if (!(layout.kind == NwDirsLayout::kUniform && cut_whole_rounds(n, nb, kHostBlk, n_sub, bcut)))
      bcut = cut_at_equal_cells(hb->cells_at.data(), nb, mat_total, n_sub);
    for (uint64_t bi : bcut) cut.push_back(hb->pair_at(bi));
  } else {
    cut = cut_at_equal_cells(h.mat_off, n, mat_total, n_sub);
  }
  NwPipeline p(ctx, std::move(cut), use_dirs && ctx->opt.walk_overlap);
  if ((rc = p.create_events())) return rc;

  // ragged chunk for the packed fill: the sub-batches' lists are made in parallel, each in its own stretch of the list -- paired
  // up by shape (moves) or the majority shape's pairs first (strings)
  std::vector<uint32_t> paired_end(n_sub, 0);   // how many of sub-batch s's list entries go two per wave
  const uint32_t *dv_list = nullptr;
  if (layout.kind == NwDirsLayout::kMixed) {
    if ((rc = ctx->h_misc.reserve(n * 4 + 16)) || (!zc_in && (rc = ctx->pair_list.reserve(n * 4 + 16)))) return rc;
    uint32_t *h_list = ctx->h_misc.as<uint32_t>();
    parallel_for(n_sub, [&](uint64_t s) {
      paired_end[s] = moves ? pair_up_shapes(h.len_a, h.len_b, p.cut[s], p.cut[s + 1], c.max_a, c.max_b, h_list + p.cut[s], false)
                            : list_majority_first(h.len_a, h.len_b, p.cut[s], p.cut[s + 1], layout.pack_a, layout.pack_b, h_list + p.cut[s]);
    });
    if (zc_in) dv_list = ctx->h_misc.dev_as<uint32_t>();
    else { dv_list = ctx->pair_list.as<uint32_t>(); HIP_TRY(hipMemcpyAsync(ctx->pair_list.p, h_list, n * 4, hipMemcpyHostToDevice, p.su)); }
  }

  // the descriptors on their way to the device
  if (!moves) {
    // ahead of the sequences on the upload stream
    HIP_TRY(hipMemcpyAsync(ctx->off_a.p, h.off_a, desc_bytes, hipMemcpyHostToDevice, p.su));
  } else if (!zc_in && layout.kind == NwDirsLayout::kUniform) {
    // one shape: the device writes them itself, in the fills' stream (uniform_descriptors_kernel)
    hipLaunchKernelGGL(uniform_descriptors_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, p.sf, ctx->off_a.as<uint64_t>(),
                       n, c.max_a, c.max_b, layout.stride);
    HIP_TRY(hipGetLastError());
    if (p.sw != p.sf) {
      HIP_TRY(hipEventRecord(p.descriptors_up(), p.sf));
      HIP_TRY(hipStreamWaitEvent(p.sw, p.descriptors_up(), 0));
    }
  } else if (!zc_in) {
    // the descriptor arrays (44 B per pair: C5's share 5.5 MB, more than a sub-batch's sequences) go up on the download
    // stream, which has nothing to do yet, beside the first sub-batch's sequences on the upload stream: two copy engines
    // (C5's share 4.2 -> 4.05 ms against the same copy ahead of the sequences on the upload stream)
    HIP_TRY(hipMemcpyAsync(ctx->off_a.p, h.off_a, desc_bytes, hipMemcpyHostToDevice, p.sd));
    HIP_TRY(hipEventRecord(p.descriptors_up(), p.sd));
    HIP_TRY(hipStreamWaitEvent(p.sf, p.descriptors_up(), 0));
    if (p.sw != p.sf) HIP_TRY(hipStreamWaitEvent(p.sw, p.descriptors_up(), 0));
  }

  const DescBlock dv(zc_in ? ctx->h_desc.dev : ctx->off_a.p, n, true);
  const uint8_t *dv_seq = zc_in ? ctx->h_arena.dev_as<uint8_t>() : ctx->arena.as<uint8_t>();
  char *dv_res = zc_out ? ctx->h_ta.dev_as<char>() : ctx->t_out_a.as<char>(), *h_res = ctx->h_ta.as<char>();
  uint32_t *dv_meta = zc_out ? ctx->h_tmeta.dev_as<uint32_t>() : ctx->t_meta.as<uint32_t>(), *h_meta = ctx->h_tmeta.as<uint32_t>();
  uint8_t *dirs = ctx->dirs.as<uint8_t>();
  int32_t *end_score = ctx->best_score.as<int32_t>();
  uint64_t *end_state = ctx->best_index.as<uint64_t>();
  auto dev_range = [&](uint64_t k0, uint64_t k1) {
    return moves ? dv.range(k0, k1, dv_seq, nullptr, nullptr, nullptr, ctx->status.as<uint64_t>(), c.max_a, c.max_b)
                 : dv.range(k0, k1, dv_seq, ctx->M.as<int32_t>(), ctx->A.as<int32_t>(), ctx->B.as<int32_t>(), ctx->status.as<uint64_t>(), c.max_a, c.max_b);
  };
  tm.lap(moves ? "nw moves: sizes, offsets, buffers" : "nw pipelined: sizes, offsets, buffers");

  // ---- enqueue: per sub-batch pack, upload, fill; per group walk and send home
  uint32_t g = 0;
  for (uint32_t s = 0; s < n_sub; ++s) {
    const uint64_t k0 = p.cut[s], k1 = p.cut[s + 1];
    if (k1 > k0) {
      if (moves) {
        // host: this sub-batch's sequences into the pinned arena, and up -- in SLICES (round 5): a slice's copy to the device runs
        // beside the packing of the next one.  C2's single sub-batch packed for 42 us and then uploaded for 72 (3 MB at 42 GB/s)
        // before its fill could start; in four slices of quarter-block tasks the last byte is up ~20 us after the last one is packed.
        const uint64_t b0 = bcut[s], n_blocks = bcut[s + 1] - b0;
        const uint64_t n_slices = zc_in ? 1 : std::min<uint64_t>(ctx->opt.upload_slices ? ctx->opt.upload_slices : 1, std::max<uint64_t>(1, n_blocks / 2));
        for (uint64_t sl = 0; sl < n_slices; ++sl) {
          const uint64_t sb0 = b0 + n_blocks * sl / n_slices, sb1 = b0 + n_blocks * (sl + 1) / n_slices;
          hb->pack(h, h_seq, sb0, sb1);
          const uint64_t c0 = h.slot[hb->pair_at(sb0)], c1 = h.slot[hb->pair_at(sb1)];
          // (tried for C2's single sub-batch: the sequences in two halves on the upload and the download stream -- the runtime
          // runs both host-to-device copies on one engine, 39 + 38 us one after the other instead of 72)
          if (!zc_in && c1 > c0) HIP_TRY(hipMemcpyAsync(ctx->arena.as<uint8_t>() + c0, h_seq + c0, c1 - c0, hipMemcpyHostToDevice, p.su));
        }
      } else {
        pack_range(batch, c.first, h, h_seq, k0, k1, 1024);
        const uint64_t c0 = h.slot[k0], c1 = h.slot[k1];
        if (c1 > c0) HIP_TRY(hipMemcpyAsync(ctx->arena.as<uint8_t>() + c0, h_seq + c0, c1 - c0, hipMemcpyHostToDevice, p.su));
      }
      if (!zc_in) {
        HIP_TRY(hipEventRecord(p.uploaded(s), p.su));
        HIP_TRY(hipStreamWaitEvent(p.sf, p.uploaded(s), 0));
      }
      const seqalign_dev_batch_t d = dev_range(k0, k1);
      if (!use_dirs) {
        if ((rc = seqalign_fill_batch_device(ctx, sc, &d, SEQALIGN_KERNEL_AUTO, p.sf))) return rc;
      } else if (layout.kind == NwDirsLayout::kMixed) {
        // one launch over the whole chunk's arrays with this sub-batch's list: the paired pairs two per wave, the others one per
        // wave, side by side in one grid
        const seqalign_dev_batch_t dm = dev_range(0, n);
        if ((rc = nw_dirs_fill_mixed(ctx, sc, &dm, dirs, end_score, end_state, p.sf, dv_list + k0, paired_end[s],
                                     (uint32_t)(k1 - k0) - paired_end[s], layout.pack_a, layout.pack_b, local)))
          return rc;
      } else {
        bool used = false;
        if ((rc = nw_dirs_fill(ctx, sc, &d, dirs, end_score + k0, end_state + k0, p.sf, &used, layout.stride, nullptr, 0, local))) return rc;
        if (!used) { set_last_error("seqalign_nw_batch: internal error: directions-only fill refused a batch it had accepted"); return SEQALIGN_E_HIP; }
      }
    }
    if (s + 1 != p.gcut[g + 1]) continue;
    // the group is filled: walk it, send it home
    const uint64_t g0 = p.cut[p.gcut[g]], g1 = k1;
    if (g1 > g0) {
      const uint64_t c0 = h.slot[g0], c1 = h.slot[g1];
      const seqalign_dev_batch_t d = dev_range(g0, g1);
      SaTraceParams t = trace_params(ctx, sc, d);
      t.str_off = dv.slot + g0; t.fill_status = d.status; t.n_pairs = (uint32_t)(g1 - g0);
      if (use_dirs) { t.dirs = dirs; t.dirs_blocked = layout.blocked; t.nw_score = end_score + g0; t.nw_state = end_state + g0; }
      if (moves) {
        t.stage_words = (c.max_a + c.max_b + 31u) >> 5;
        t.moves = reinterpret_cast<uint32_t *>(dv_res) + 2 * g0;   // walk w of the launch is pair g0 + w: words 2 ((slot >> 5) + g0 + w)
        t.out_meta2 = dv_meta + 2 * g0;
        t.dirs_local = local; t.tune_stage = ctx->opt.walk_stage; t.tune_tile = ctx->opt.walk_tile;
      } else {
        t.M = d.match_scores; t.A = d.gap_a_scores; t.B = d.gap_b_scores;
        t.out_a = dv_res + 2 * c0 - c0;                  // + slot offset: a-strings at [2 c0, 2 c0 + (c1 - c0))
        t.out_b = dv_res + 2 * c0 + (c1 - c0) - c0;      //                b-strings right behind them
        t.out_meta4 = dv_meta + 4 * g0;
      }
      hipStream_t sg = p.walk_stream(g);
      if (sg != p.sf) {
        HIP_TRY(hipEventRecord(p.filled(g), p.sf));
        HIP_TRY(hipStreamWaitEvent(sg, p.filled(g), 0));
      }
      hipError_t e = sa_launch_nw_traceback(t, sg);
      if (e != hipSuccess) return fail_hip(e, "traceback launch");
      if (zc_out) {
        HIP_TRY(hipEventRecord(p.home(g), sg));
      } else {
        HIP_TRY(hipEventRecord(p.walked(g), sg));
        HIP_TRY(hipStreamWaitEvent(p.sd, p.walked(g), 0));
        if (moves) {
          const uint64_t w0 = h.move_word(g0), w1 = g1 < n ? h.move_word(g1) : move_words - 2;
          HIP_TRY(hipMemcpyAsync(h_res + w0 * 4, dv_res + w0 * 4, (w1 - w0) * 4, hipMemcpyDeviceToHost, p.sd));
          HIP_TRY(hipMemcpyAsync(h_meta + 2 * g0, dv_meta + 2 * g0, (g1 - g0) * 8, hipMemcpyDeviceToHost, p.sd));
        } else {
          if (c1 > c0) HIP_TRY(hipMemcpyAsync(h_res + 2 * c0, dv_res + 2 * c0, 2 * (c1 - c0), hipMemcpyDeviceToHost, p.sd));
          HIP_TRY(hipMemcpyAsync(h_meta + 4 * g0, dv_meta + 4 * g0, (g1 - g0) * 16, hipMemcpyDeviceToHost, p.sd));
        }
        HIP_TRY(hipEventRecord(p.home(g), p.sd));
      }
    } else {
      HIP_TRY(hipEventRecord(p.home(g), p.sf));
    }
    ++g;
  }
  tm.lap(moves ? "nw moves: packed + enqueued" : "nw pipelined: all sub-batches packed + enqueued");

  // ---- deliver: the groups in order, as they land, into the caller's buffers
  LowestFailure bad;
  double wait_ms = 0, copy_ms = 0;   // (strings, option timing: the lap below divided into waiting for the GPU / copying out)
  auto now_ms = [] { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; };
  const MovesHome home{batch, c.first, h, reinterpret_cast<const uint32_t *>(h_res), h_meta, ctx->cigar_format, ctx->cigar_fold,
                       str_off, out_a, out_b, out_len, out_score};
  for (g = 0; g < p.n_grp; ++g) {
    const uint64_t k_lo = p.cut[p.gcut[g]], k_hi = p.cut[p.gcut[g + 1]];
    if (moves) {
      { const hipError_t e = wait_event_spinning(p.home(g)); if (e != hipSuccess) return fail_hip(e, "waiting for a group's walk"); }
      expand_moves(home, k_lo, k_hi, bad);
      continue;
    }
    const double t_w = now_ms();
    HIP_TRY(hipEventSynchronize(p.home(g)));
    const double t_c = now_ms();
    wait_ms += t_c - t_w;
    if (k_hi == k_lo) continue;
    // strings of group g from the pinned block into the caller's buffers
    const uint64_t c0 = h.slot[k_lo], c1 = h.slot[k_hi], first = c.first;
    const char *ha = h_res + 2 * c0 - c0, *hb_ = h_res + 2 * c0 + (c1 - c0) - c0;   // + slot offset
    constexpr uint64_t kPack = 1024;
    parallel_for((k_hi - k_lo + kPack - 1) / kPack, [=, &bad](uint64_t blk_i) {
      for (uint64_t k = k_lo + blk_i * kPack, e = std::min(k_hi, k_lo + (blk_i + 1) * kPack); k < e; ++k) {
        const uint64_t pr = first + k;
        const uint32_t head = h_meta[4 * k], len = h_meta[4 * k + 1], status = h_meta[4 * k + 3];
        if (status) { bad.note(k, (int)(status & 255u)); continue; }
        memcpy(out_a + str_off[pr], ha + h.slot[k] + head, len);   // left-align (needleman_wunsch.c:135-145)
        memcpy(out_b + str_off[pr], hb_ + h.slot[k] + head, len);
        out_a[str_off[pr] + len] = out_b[str_off[pr] + len] = '\0';
        out_len[pr] = len;
        out_score[pr] = (int32_t)h_meta[4 * k + 2];
      }
    });
    copy_ms += now_ms() - t_c;
  }
  if (bad.code()) return bad.code();
  if (!moves && ctx->opt.timing) fprintf(stderr, "[seqalign timing] nw pipelined: waiting for the groups %.3f ms, copying their strings out %.3f ms\n", wait_ms, copy_ms);
  tm.lap(moves ? "nw moves: groups expanded" : "nw pipelined: all groups unpacked");
  return SEQALIGN_OK;
}

// The HOST legs of the moves form alone -- sizes, offsets, packing the sequences; then the expansion of (synthetic: all MATCH)
// moves into the caller's strings -- with no device involved: what a rank's CPU share must sustain per call when eight ranks do
// this at once on two sockets (tools/host_scale.py).  Plain memory instead of pinned; the loops are the shipped ones (scan_blocks,
// HostBlocks::place / pack with their quarter-block tasks, expand_moves with its prefetch) on the ragged layout, same pool.
extern "C" int seqalign_host_legs_nw(const seqalign_batch_t *batch, const uint64_t *str_off, char *out_a, char *out_b,
                                     uint32_t *out_len, int iterations, double *pack_ms, double *expand_ms) {
  if (!batch || !str_off || !out_a || !out_b || !out_len || iterations <= 0 || !pack_ms || !expand_ms) return SEQALIGN_E_ARG;
  const uint64_t n = batch->n_pairs, kHostBlk = 512;
  if (!n) return SEQALIGN_OK;
  std::vector<BlkSum> blk;
  std::vector<uint64_t> desc(DescBlock::bytes(n, true) / 8 + 1);
  const DescBlock h(desc.data(), n, true);
  std::vector<uint8_t> seq;
  std::vector<uint32_t> moves, meta(2 * n);
  std::vector<int32_t> score(n);
  for (uint64_t k = 0; k < n; ++k) { meta[2 * k] = 0; meta[2 * k + 1] = std::min(batch->len_a[k], batch->len_b[k]); }
  NwDirsLayout layout;
  layout.kind = NwDirsLayout::kMixed;
  auto now_ms = [] { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; };
  double t_pack = 0, t_expand = 0;
  for (int it = 0; it < iterations; ++it) {
    const double t0 = now_ms();
    scan_blocks(batch, 0, n, kHostBlk, blk);
    const HostBlocks hb(batch, 0, n, kHostBlk, blk, layout);
    const uint64_t total = hb.chars_at.back();
    if (seq.size() < total + 64) seq.resize(total + 64);
    if (moves.size() < 2 * ((total >> 5) + n) + 2) moves.assign(2 * ((total >> 5) + n) + 2, 0u);
    hb.place(h, layout);
    hb.pack(h, seq.data(), 0, blk.size());
    const double t1 = now_ms();
    LowestFailure bad;
    expand_moves(MovesHome{batch, 0, h, moves.data(), meta.data(), 0, false, str_off, out_a, out_b, out_len, score.data()}, 0, n, bad);
    const double t2 = now_ms();
    if (bad.code()) return SEQALIGN_E_TRACEBACK;
    t_pack += t1 - t0; t_expand += t2 - t1;
  }
  *pack_ms = t_pack / iterations; *expand_ms = t_expand / iterations;
  return SEQALIGN_OK;
}


// (CIGAR mode -- ctx->cigar_format, set by seqalign_nw_batch_cigar: only the direction-byte path, whose walks come home as bit
// planes, delivers it; for every other path kNeedsStrings tells the caller to run the call for strings and convert them)
static constexpr int kNeedsStrings = -1;
static int nw_batch_impl(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                         const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len,
                         int32_t *out_score) {
  const seqalign_batch_t *b = batch;
  if (!batch_readable(b)) return SEQALIGN_E_ARG;
  if (batch->n_pairs == 0) return SEQALIGN_OK;
  int rc;
  // one parallel pass over the lengths: validity (check_batch) and the sizes chunk planning needs
  std::vector<BlkSum> blk;
  const uint64_t blk_pairs = host_block_pairs(ctx, batch->n_pairs);
  scan_blocks(batch, 0, batch->n_pairs, blk_pairs, blk);
  Chunk whole;
  whole.count = batch->n_pairs;
  uint64_t cells256 = 0;
  for (const BlkSum &s : blk) {
    if (s.too_large) return SEQALIGN_E_TOO_LARGE;
    whole.cells += s.cells; whole.seq_bytes += s.chars; cells256 += std::max(s.cells256, s.blk256);   // (the larger of the two layouts' bytes: which one a chunk takes follows from its widest row)
    whole.max_a = std::max(whole.max_a, s.max_a); whole.max_b = std::max(whole.max_b, s.max_b);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  seqalign_dev_scoring *sc = nullptr;
  if ((rc = cached_scoring(ctx, scoring, 0, &sc))) return rc;
  if ((rc = admit_magnitude(sc, whole.max_a, whole.max_b, SA_FRAMES_FILL))) return rc;
  const bool on_host = traceback_on_host(ctx);
  if (!on_host && ctx->opt.nw_moves && nw_dirs_applicable(ctx, sc, whole.max_a, batch->n_pairs)) {
    // direction bytes (1 B per cell, every pair rounded up to 256 at most) + ~64 B per pair of descriptors and results:
    // C5's 1 M pairs are 23 GB -- one chunk, where 12 B per cell cut them into six
    if (cells256 + 64 * batch->n_pairs + whole.seq_bytes <= ctx->chunk_budget)
      return nw_chunk(ctx, batch, whole, sc, &blk, blk_pairs, str_off, out_a, out_b, out_len, out_score);
    std::vector<uint64_t> extra(batch->n_pairs, 256 + 64);
    if (SA_DIRS_BLOCKED)   // (in blocks of 8 x 16 cells a pair's direction bytes are up to 8 columns' + 16 rows' worth more than its cells)
      for (uint64_t p = 0; p < batch->n_pairs; ++p) {
        const uint64_t cells = (uint64_t)(batch->len_a[p] + 1ull) * (batch->len_b[p] + 1ull), bb = sa_dirs_blocked_bytes(batch->len_a[p], batch->len_b[p]);
        if (bb > cells) extra[p] += bb - cells;
      }
    for (const Chunk &c : plan_chunks(batch, ctx->chunk_budget, 1, extra.data())) {
      const uint64_t bp = host_block_pairs(ctx, c.count);
      scan_blocks(batch, c.first, c.count, bp, blk);
      if ((rc = nw_chunk(ctx, batch, c, sc, &blk, bp, str_off, out_a, out_b, out_len, out_score))) return rc;
    }
    return SEQALIGN_OK;
  }
  if (ctx->cigar_format) return kNeedsStrings;
  // host mode: matrices come back through pinned staging, so chunks are also bounded by host memory
  const size_t budget = on_host ? std::min<size_t>(ctx->chunk_budget, (size_t)6 << 30) : ctx->chunk_budget;
  for (const Chunk &c : plan_chunks(batch, budget)) {
    seqalign_dev_batch_t d;
    if (!on_host) {
      // (one sub-batch = the plain sequence upload, fill, walk, download on the same code path)
      if ((rc = nw_chunk(ctx, batch, c, sc, nullptr, 0, str_off, out_a, out_b, out_len, out_score))) return rc;
      continue;
    }
    if ((rc = run_chunk(ctx, batch, c, sc, &d))) return rc;
    const size_t bytes = c.cells * 4;
    if ((rc = ctx->h_M.reserve(bytes)) || (rc = ctx->h_A.reserve(bytes)) || (rc = ctx->h_B.reserve(bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(ctx->h_M.p, ctx->M.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_A.p, ctx->A.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_B.p, ctx->B.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = fetch_status(ctx, c, nullptr))) return rc;   // syncs; unknown pair is fatal for NW
    std::vector<uint64_t> cell0(c.count);
    { uint64_t cell = 0;
      for (uint64_t k = 0; k < c.count; ++k) {
        cell0[k] = cell;
        cell += (uint64_t)(batch->len_a[c.first + k] + 1ull) * (batch->len_b[c.first + k] + 1ull);
      } }
    std::atomic<int> first_error{SEQALIGN_OK};
    parallel_for(c.count, [&](uint64_t k) {
      const uint64_t p = c.first + k;
      sa_view_t v;
      v.sc = scoring; v.a = batch->arena + batch->off_a[p]; v.b = batch->arena + batch->off_b[p];
      v.len_a = batch->len_a[p]; v.len_b = batch->len_b[p];
      v.M = ctx->h_M.as<int32_t>() + cell0[k]; v.A = ctx->h_A.as<int32_t>() + cell0[k];
      v.B = ctx->h_B.as<int32_t>() + cell0[k];
      size_t n = 0;
      int prc = sa_nw_traceback(&v, out_a + str_off[p], out_b + str_off[p], &n, &out_score[p]);
      out_len[p] = (uint32_t)n;
      if (prc != SEQALIGN_OK) { int expected = SEQALIGN_OK; first_error.compare_exchange_strong(expected, prc); }
    });
    if ((rc = first_error.load())) return rc;
  }
  return SEQALIGN_OK;
}

extern "C" int seqalign_nw_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                 const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len,
                                 int32_t *out_score) {
  if (!ctx || !scoring || !str_off || !out_a || !out_b || !out_len || !out_score) return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  return nw_batch_impl(ctx, batch, scoring, str_off, out_a, out_b, out_len, out_score);
}

uint64_t sa_host::put_alignment(const seqalign_ctx *ctx, const char *sa, const char *sb, uint32_t len, char *out_a, char *out_b,
                                uint64_t at, uint64_t room) {
  if (!ctx->cigar_format) {
    if ((uint64_t)len + 1 > room) return 0;
    memcpy(out_a + at, sa, len); memcpy(out_b + at, sb, len);
    out_a[at + len] = out_b[at + len] = '\0';
    return (uint64_t)len + 1;
  }
  if (!room) return 0;
  const size_t n = seqalign_cigar(sa, sb, len, ctx->cigar_format == 2, ctx->cigar_fold, out_a + at, room);
  return n == (size_t)-1 ? 0 : (uint64_t)n + 1;
}

// Global alignments as CIGAR (include/seqalign_hip.h).  On the direction-byte path the walks come home as two bit planes and the
// host run-length encodes those (host/sa_moves.c: sa_cigar_nw_moves): no string is ever written.  The other paths (three
// matrices, traceback = host) produce strings: the call runs for strings into its own buffers and encodes them.
extern "C" int seqalign_nw_batch_cigar(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int format,
                                       const uint64_t *cigar_off, char *cigar, uint32_t *cigar_len, int32_t *out_score) {
  if (!ctx || !scoring || !cigar_off || !cigar || !cigar_len || !out_score || (format != SEQALIGN_CIGAR_M && format != SEQALIGN_CIGAR_EQX))
    return SEQALIGN_E_ARG;
  CallScope scope(ctx);
  if (!batch) return SEQALIGN_E_ARG;
  for (uint64_t p = 0; p < batch->n_pairs; ++p)
    if (cigar_off[p + 1] < cigar_off[p]) return SEQALIGN_E_ARG;
  int rc;
  {
    CigarScope mode(ctx, format, !scoring->case_sensitive);
    rc = nw_batch_impl(ctx, batch, scoring, cigar_off, cigar, cigar, cigar_len, out_score);
  }
  if (rc != kNeedsStrings) return rc;
  const uint64_t n = batch->n_pairs;
  std::vector<uint64_t> off(n + 1, 0);
  for (uint64_t p = 0; p < n; ++p) off[p + 1] = off[p] + batch->len_a[p] + batch->len_b[p] + 1;
  std::vector<char> sa(off[n] + 1), sb(off[n] + 1);
  std::vector<uint32_t> len(n);
  if ((rc = nw_batch_impl(ctx, batch, scoring, off.data(), sa.data(), sb.data(), len.data(), out_score))) return rc;
  LowestFailure bad;
  parallel_for((n + 255) / 256, [&](uint64_t blk) {
    for (uint64_t p = blk * 256, e = std::min(n, (blk + 1) * 256); p < e; ++p) {
      const uint64_t cap = cigar_off[p + 1] - cigar_off[p];
      const size_t got = cap ? seqalign_cigar(sa.data() + off[p], sb.data() + off[p], len[p], format == SEQALIGN_CIGAR_EQX,
                                              !scoring->case_sensitive, cigar + cigar_off[p], cap) : (size_t)-1;
      if (got == (size_t)-1) bad.note(p, SEQALIGN_E_NOMEM);
      else cigar_len[p] = (uint32_t)got;
    }
  });
  return bad.code();
}
