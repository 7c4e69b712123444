// sa_chunks.hpp -- the chunk driver of the host-level calls whose chunks are cut by device BYTES: score only
// (sa_batch_score.hip, which also holds the span call) and the banded calls (sa_batch_band.hip).  Host code only.
//   cut_chunks        the batch cut into ranges of pairs that fit the context's chunk budget
//   ChunkStage        one chunk on its way up: its pairs sorted into launch classes, the descriptors laid out in slot
//                     order, the sequences packed in pair order, both uploaded; and on the way back the lowest failing
//                     pair found from the status words and the results put back in pair order
//   time_launches     a launch repeated between HIP events (the *_time_ms hooks)
// What a call's kernels need besides -- result and scratch buffers, further descriptor arrays -- stays with the call.
#pragma once
#include "sa_ctx.hpp"

namespace sa_host {

constexpr uint64_t kChunkMaxPairs = (uint64_t)1 << 24;

struct ByteChunk {
  uint64_t first = 0, count = 0;       // pairs [first, first + count)
  uint64_t seq_bytes = 0, cells = 0;   // sums of len_a + len_b and of PairNeed::cells
};

// What one pair adds to its chunk: device bytes; cells, summed per chunk for the caller; and rows of a launch grid that is
// (the chunk's pairs rounded up to 8, one spare) x (its largest `grid_rows`) workgroups.  Callers without such a grid leave 0.
struct PairNeed {
  uint64_t bytes = 0, cells = 0, grid_rows = 0;
};

// Greedy cut in pair order: a chunk is closed before the pair that would take its bytes over `budget`, its pairs over
// kChunkMaxPairs or its grid over `grid_max` workgroups.  A pair whose bytes alone exceed the budget is a chunk of its own,
// or, with refuse_oversize, SEQALIGN_E_NOMEM with the bytes named.
template <class Need>
int cut_chunks(const seqalign_batch_t *b, size_t budget, Need need_of, std::vector<ByteChunk> &out, bool refuse_oversize = false,
               uint64_t grid_max = ~(uint64_t)0) {
  ByteChunk c;
  uint64_t used = 0, rows_max = 0;
  for (uint64_t p = 0; p < b->n_pairs; ++p) {
    const PairNeed need = need_of(p);
    if (refuse_oversize && need.bytes > budget) {
      set_last_error("pair " + std::to_string(p) + ": " + std::to_string(need.bytes) + " bytes of device memory needed, the chunk budget is " +
                     std::to_string(budget));
      return SEQALIGN_E_NOMEM;
    }
    if (c.count && (used + need.bytes > budget || c.count == kChunkMaxPairs ||
                    ((c.count + 8) & ~(uint64_t)7) * std::max(rows_max, need.grid_rows) > grid_max)) {
      out.push_back(c); c = ByteChunk(); c.first = p; used = 0; rows_max = 0;
    }
    rows_max = std::max(rows_max, need.grid_rows);
    used += need.bytes;
    c.count++; c.seq_bytes += (uint64_t)b->len_a[p] + b->len_b[p];
    c.cells += need.cells;
  }
  if (c.count) out.push_back(c);
  return SEQALIGN_OK;
}

// One chunk staged for kernels that take one launch per class of CLASSES + 1 (sort_by_class, sa_ctx.hpp).
// The private descriptor block, pinned (ctx->h_desc) and on the device (ctx->off_a), in slot order, n entries per array:
//   off_a, off_b, the caller's n_u64 arrays (uint64_t), len_a, len_b, the caller's n_u32 arrays (32 bits)
// The sequences go to ctx->h_arena / ctx->arena in pair order; ctx->status has a word per slot.
template <int CLASSES>
struct ChunkStage {
  seqalign_ctx *ctx = nullptr;
  uint64_t n = 0, first = 0, seq_bytes = 0;
  std::vector<uint32_t> order;           // descriptor slot -> pair of the chunk
  uint64_t cls_first[CLASSES + 2] = {};  // class x: slots [cls_first[x], cls_first[x + 1])
  uint32_t cls_max[CLASSES + 1] = {};    // its largest key
  int n_u64 = 0, n_u32 = 0;
  uint64_t *h_off_a = nullptr, *h_off_b = nullptr, *d_off_a = nullptr, *d_off_b = nullptr;
  uint32_t *h_len_a = nullptr, *h_len_b = nullptr, *d_len_a = nullptr, *d_len_b = nullptr;

  // the caller's arrays, pinned and on the device
  uint64_t *h_u64(int i) const { return h_off_a + (2 + i) * n; }
  uint64_t *d_u64(int i) const { return d_off_a + (2 + i) * n; }
  template <class T = uint32_t> T *h_u32(int i) const { return reinterpret_cast<T *>(h_len_a + (2 + i) * n); }
  template <class T = uint32_t> T *d_u32(int i) const { return reinterpret_cast<T *>(d_len_a + (2 + i) * n); }
  size_t desc_bytes() const { return n * ((2 + n_u64) * sizeof(uint64_t) + (2 + n_u32) * sizeof(uint32_t)); }
  uint64_t class_size(int x) const { return cls_first[x + 1] - cls_first[x]; }

  // The host side: the chunk's pairs sorted by cls_of(key(p)), the shared descriptors filled slot by slot -- fill_slot(s, p)
  // follows each with the caller's arrays of slot s, batch pair p -- and the sequences packed; the device buffers reserved.
  template <class Cls, class Key, class FillSlot>
  int lay_out(const seqalign_batch_t *b, const ByteChunk &c, Cls cls_of, Key key, int extra_u64, int extra_u32, FillSlot fill_slot) {
    int rc;
    n = c.count; first = c.first; seq_bytes = c.seq_bytes;
    n_u64 = extra_u64; n_u32 = extra_u32;
    order.resize(n);
    sort_by_class<CLASSES>(n, cls_of, [&](uint64_t k) { return key(first + k); }, order.data(), cls_first, cls_max);
    if ((rc = ctx->h_desc.reserve(desc_bytes())) || (rc = ctx->h_arena.reserve(seq_bytes + 16))) return rc;
    h_off_a = ctx->h_desc.as<uint64_t>(); h_off_b = h_off_a + n;
    h_len_a = reinterpret_cast<uint32_t *>(h_off_a + (2 + n_u64) * n); h_len_b = h_len_a + n;
    std::vector<uint64_t> seq_at(n);
    { uint64_t pos = 0;
      for (uint64_t k = 0; k < n; ++k) { seq_at[k] = pos; pos += (uint64_t)b->len_a[first + k] + b->len_b[first + k]; } }
    for (uint64_t s = 0; s < n; ++s) {
      const uint64_t k = order[s], p = first + k;
      h_off_a[s] = seq_at[k]; h_off_b[s] = seq_at[k] + b->len_a[p];
      h_len_a[s] = b->len_a[p]; h_len_b[s] = b->len_b[p];
      fill_slot(s, p);
    }
    uint8_t *h_seq = ctx->h_arena.as<uint8_t>();
    constexpr uint64_t kTask = 256;
    parallel_for((n + kTask - 1) / kTask, [&](uint64_t blk) {
      for (uint64_t k = blk * kTask, e = std::min(n, (blk + 1) * kTask); k < e; ++k) {
        const uint64_t p = first + k;
        memcpy(h_seq + seq_at[k], b->arena + b->off_a[p], b->len_a[p]);
        memcpy(h_seq + seq_at[k] + b->len_a[p], b->arena + b->off_b[p], b->len_b[p]);
      }
    });
    if ((rc = ctx->arena.reserve(seq_bytes + 16)) || (rc = ctx->off_a.reserve(desc_bytes())) || (rc = ctx->status.reserve(n * 8))) return rc;
    d_off_a = ctx->off_a.as<uint64_t>(); d_off_b = d_off_a + n;
    d_len_a = reinterpret_cast<uint32_t *>(d_off_a + (2 + n_u64) * n); d_len_b = d_len_a + n;
    return SEQALIGN_OK;
  }

  // descriptors and sequences on their way up, on ctx->stream
  int upload() {
    HIP_TRY(hipMemcpyAsync(ctx->off_a.p, h_off_a, desc_bytes(), hipMemcpyHostToDevice, ctx->stream));
    if (seq_bytes) HIP_TRY(hipMemcpyAsync(ctx->arena.p, ctx->h_arena.p, seq_bytes, hipMemcpyHostToDevice, ctx->stream));
    return SEQALIGN_OK;
  }

  // the kernels' common arguments of slots [s0, s0 + m)
  void set_slots(SaFillParams &f, uint64_t s0, uint64_t m) const {
    f.arena = ctx->arena.as<uint8_t>();
    f.off_a = d_off_a + s0; f.off_b = d_off_b + s0; f.len_a = d_len_a + s0; f.len_b = d_len_b + s0;
    f.status = ctx->status.as<uint64_t>() + s0;
    f.n_pairs = (uint32_t)m;
  }

  // SEQALIGN_E_UNKNOWN_PAIR for the lowest pair of the chunk whose status word names a cell (the stream is idle)
  int fail_from_status(uint64_t *fail_pair = nullptr) const {
    std::vector<uint64_t> status(n);
    HIP_TRY(hipMemcpy(status.data(), ctx->status.p, 8 * n, hipMemcpyDeviceToHost));
    uint64_t worst = ~0ull;
    for (uint64_t s = 0; s < n; ++s)
      if (status[s] != ~0ull) worst = std::min<uint64_t>(worst, order[s]);
    if (fail_pair) *fail_pair = first + worst;
    return fail_unknown_pair(first + worst);
  }

  // results that came home as `fields` arrays of n words in slot order, put into the caller's arrays in pair order: array 0
  // to out_score, array f to out[f - 1]
  void scatter(const uint32_t *h, int fields, int32_t *out_score, uint32_t *const *out) const {
    constexpr uint64_t kTask = 16384;
    parallel_for((n + kTask - 1) / kTask, [&](uint64_t blk) {
      for (uint64_t s = blk * kTask, e = std::min(n, (blk + 1) * kTask); s < e; ++s) {
        const uint64_t p = first + order[s];
        out_score[p] = (int32_t)h[s];
        for (int f = 1; f < fields; ++f) out[f - 1][p] = h[(uint64_t)f * n + s];
      }
    });
  }
};

// launch() enqueued `repeats` times on `st`, each between two HIP events: ms_each[r] = what the r-th took on the device
template <class Launch>
int time_launches(hipStream_t st, int repeats, float *ms_each, Launch launch) {
  int rc;
  EventList events;
  for (int r = 0; r < 2 * repeats; ++r) HIP_TRY(events.add());
  for (int r = 0; r < repeats; ++r) {
    HIP_TRY(hipEventRecord(events.ev[2 * r], st));
    if ((rc = launch())) return rc;
    HIP_TRY(hipEventRecord(events.ev[2 * r + 1], st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  for (int r = 0; r < repeats; ++r) HIP_TRY(hipEventElapsedTime(&ms_each[r], events.ev[2 * r], events.ev[2 * r + 1]));
  return SEQALIGN_OK;
}

}  // namespace sa_host
