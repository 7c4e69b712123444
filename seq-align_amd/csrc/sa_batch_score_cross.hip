// sa_batch_score_cross.hip -- score matrices: seqalign_nw_score_cross / seqalign_sw_score_cross, every query of one set
// against every target of another, score only.  The result is seqalign_*_score_batch's on the batch whose pair
// q * n_targets + t is (query q, target t), but that batch is never built: its descriptors and its packed sequences grow
// with Q x T, the sets themselves with Q + T.
//
// Queries of up to SA_SCORE_ROW_MAX columns: tiles of (query range x target range) within ctx->chunk_budget -- the tile's
// sequences, their descriptors and 4 (NW) / 12 (SW) bytes of results per pair.  Usually every target fits one range and a
// tile is a query range; the targets then go up once per call.  Per tile: each sequence uploaded once, one
// score_cross_kernel launch per row class of its queries (sa_score.hip: wave -> (query, target), longest targets first),
// the result rows home and copied row by row into the caller's matrix.  A failing pair leaves its tile-local index
// q * n_t + t in one 64-bit atomicMin; a tile's order is the matrix's row-major order restricted to the tile, so the lowest
// tile-local index is the tile's lowest failing pair, and the call's is the lowest over the tiles of the first query range
// that has one.
//
// Longer queries: seqalign_*_score_batch's strips, on explicit pair lists (a few long queries x a slice of the targets),
// results scattered into the matrix.  Such a pair is over 1 024 x len_b cells: building its descriptor costs nothing next to it.
//
// Top-k search (seqalign_*_score_search) runs the same tiles; only the end of a tile differs.  Instead of the rows going
// home, score_select_kernel (sa_score_select.hip) merges each row's best entries into its query's running list on the device
// ([nq][k] keys, ends, counts, reserved with the other buffers), and after a query range's last target range only the lists
// come home: nq x (16 k + 4) bytes.  The tile cut counts the lists as part of each query's bytes.  Long queries' rows come
// home through the score batches anyway; their top k is taken on the host with the same key.
//
// Span matrices (seqalign_sw_span_cross) are the same tiles once more with 20 result bytes per pair: the CROSS form of the span
// kernel (sa_span.hip) in place of the score kernel's, five rows home per query, and the short / long split at SA_SPAN_ROW_MAX
// columns, the long queries through the span strips (row_batch_call<SpanTraits>).
//
// Statistics matrices (seqalign_nw_stats_cross) are the span matrices' tiles with 12 result bytes per pair: the CROSS form of the
// stats kernel (sa_nw_stats.hip), three rows home per query, the same split at SA_SPAN_ROW_MAX columns, the long queries through
// the stats strips (row_batch_call<StatsTraits>).  A pair whose end pick has no walk (SA_STATS_NO_WALK) is SEQALIGN_E_TRACEBACK;
// between it and a pair without a score the lower pair's code is the call's.
//
// SW statistics matrices (seqalign_sw_stats_cross) are the span matrices' tiles once more with 28 result bytes per pair: the CROSS
// form of the SW stats kernel (sa_sw_stats.hip), seven rows home per query, the long queries through its strips
// (row_batch_call<SwStatsTraits>).  Every query and every target has at most SEQALIGN_SW_STATS_MAX_LEN letters (checked at the entry).
//
// Top-k search with spans (seqalign_sw_span_search) is two stages: the score search above, unchanged, and then
// the span sweep on the selected hits alone -- for each the PREFIX pair (query[0 : end_a], target[0 : end_b]), whose first hit
// is the full pair's, as an explicit pair list through span_batch_impl.
//
// The four families are one driver, CrossCall<R>, over the batch driver's traits structs (sa_row_families.hpp): one parameter
// block per row class, R's CROSS launch, R's result layout, R's batch call for the long queries.
#include "sa_row_families.hpp"

using namespace sa_host;

namespace {

constexpr uint64_t kSeqBytes = 16;                        // per sequence besides its bytes: offset 8, length 4, list entry 4
constexpr uint64_t kTileMaxPairs = (uint64_t)1 << 24;     // one launch's waves (as kChunkMaxPairs of the score batches)
constexpr uint64_t kLongSlicePairs = (uint64_t)1 << 16;   // pairs of one score-batch slice of the long queries

struct Range {
  uint64_t first = 0, count = 0, bytes = 0;   // into a list of sequences; bytes: their characters
};

// Cut `idx` (sequences of `s`) into ranges whose cost sum(len + kSeqBytes) + count * per_seq stays within `budget` and whose
// count stays within max_count; at least one sequence per range.
std::vector<Range> cut_ranges(const seqalign_seqset_t *s, const std::vector<uint64_t> &idx, uint64_t budget, uint64_t per_seq,
                              uint64_t max_count) {
  std::vector<Range> out;
  Range r;
  uint64_t used = 0;
  for (uint64_t k = 0; k < idx.size(); ++k) {
    const uint64_t len = s->len[idx[k]], need = len + kSeqBytes + per_seq;
    if (r.count && (used + need > budget || r.count == max_count)) { out.push_back(r); r = Range(); r.first = k; used = 0; }
    used += need;
    r.count++; r.bytes += len;
  }
  if (r.count) out.push_back(r);
  return out;
}

// the lowest failing pair of the call so far (row-major key q * n_targets + t)
struct FailPair {
  uint64_t key = ~0ull, q = 0, t = 0;
  void offer(uint64_t q_, uint64_t t_, uint64_t n_t) {
    const uint64_t k = q_ * n_t + t_;
    if (k < key) { key = k; q = q_; t = t_; }
  }
  bool any() const { return key != ~0ull; }
};

// the search's order: ascending keys are score descending, then target ascending
inline uint32_t key_u(int32_t s) { return ~((uint32_t)s ^ 0x80000000u); }
inline uint64_t hit_key(int32_t s, uint64_t t) { return ((uint64_t)key_u(s) << 32) | t; }

struct SearchOut {   // seqalign_*_score_search's outputs, or seqalign_sw_span_search's after its first stage
  uint32_t k;
  int32_t min_score;
  seqalign_search_hit_t *hits;   // [n_queries * k]
  uint32_t *n_hits;              // [n_queries]
  seqalign_span_hit_t *span_hits = nullptr;   // set: these instead of `hits`, pos 0 and len = the end cell until stage 2
  // query q's list from sorted keys and their ends
  void put(uint64_t q, uint32_t n, const uint64_t *key, const uint32_t *ea, const uint32_t *eb) const {
    n_hits[q] = n;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t target = (uint32_t)key[i];
      const int32_t score = (int32_t)(~(uint32_t)(key[i] >> 32) ^ 0x80000000u);
      if (span_hits) span_hits[q * k + i] = seqalign_span_hit_t{target, score, 0, 0, ea[i], eb[i]};
      else hits[q * k + i] = seqalign_search_hit_t{target, score, ea[i], eb[i]};
    }
  }
};

// One cross call of family R (sa_row_families.hpp): its tiles through R's CROSS kernel, its long queries through R's batch call
template <class R>
struct CrossCall {
  seqalign_ctx *ctx;
  const seqalign_seqset_t *Q, *T;
  const scoring_t *scoring;
  bool is_sw;
  int32_t *out_score;
  uint32_t *const *out_w;   // the matrices behind the score, fields() - 1 of them in R::set_results' order
  uint64_t nT;
  const SearchOut *search = nullptr;   // set: top-k search (the score family only), the matrix outputs are unused
  FailPair fail;                       // the lowest pair without a score
  FailPair no_walk;                    // R::kMarkField: the lowest pair whose end pick has no walk (SEQALIGN_E_TRACEBACK)

  int fields() const { return R::fields(is_sw); }   // result words per pair, the score first
  uint64_t result_bytes() const { return 4 * (uint64_t)fields(); }
  uint64_t list_bytes() const { return search ? 16ull * search->k + 4 : 0; }   // one query's running list

  // queries <= R::kRowMax: the cross kernel, tile by tile
  int run_short(const std::vector<uint64_t> &qs) {
    int rc;
    seqalign_dev_scoring *sc = nullptr;
    if ((rc = cached_scoring(ctx, scoring, is_sw ? 1 : 0, &sc))) return rc;
    const uint64_t budget = std::max<uint64_t>(ctx->chunk_budget, 4096), rp = result_bytes();

    std::vector<uint64_t> ts(nT);
    for (uint64_t t = 0; t < nT; ++t) ts[t] = t;
    // targets: at most half the budget in bytes, a quarter in one row of results
    const std::vector<Range> t_ranges = cut_ranges(T, ts, budget / 2, 0, std::max<uint64_t>(1, std::min(kTileMaxPairs, budget / 4 / rp)));
    uint64_t tb_max = 0, nt_max = 0;
    for (const Range &r : t_ranges) { tb_max = std::max(tb_max, r.bytes); nt_max = std::max(nt_max, r.count); }
    const uint64_t t_room = tb_max + nt_max * kSeqBytes;
    const std::vector<Range> q_ranges = cut_ranges(Q, qs, budget > t_room ? budget - t_room : 0, nt_max * rp + list_bytes(),
                                                   std::max<uint64_t>(1, kTileMaxPairs / nt_max));
    uint64_t qb_max = 0, nq_max = 0;
    for (const Range &r : q_ranges) { qb_max = std::max(qb_max, r.bytes); nq_max = std::max(nq_max, r.count); }

    // every buffer at its largest before anything goes up (a DevBuf that grows loses its contents): sequences, targets
    // first; descriptors off_t, off_q (u64), len_t, t_order, len_q, q_list (u32); results: err_flag, -, err_pair (u64), then
    // score, end_a, end_b (span: score, pos_a, pos_b, len_a, len_b); search: the running lists of a query range (keys u64
    // [nq * k], end_a, end_b u32 [nq * k], counts u32 [nq]), and at home the 16 bytes of err_flag / err_pair followed by the
    // lists
    const uint64_t q_at = (tb_max + 15) & ~(uint64_t)15;
    const uint64_t desc_bytes = 16 * (nt_max + nq_max);
    const uint64_t res_bytes = 16 + rp * nq_max * nt_max, lists_bytes = list_bytes() * nq_max;
    if ((rc = ctx->arena.reserve(q_at + qb_max + 16)) || (rc = ctx->off_a.reserve(desc_bytes)) ||
        (rc = ctx->best_score.reserve(res_bytes)) || (rc = ctx->h_arena.reserve(q_at + qb_max + 16)) ||
        (rc = ctx->h_desc.reserve(desc_bytes)) || (rc = ctx->h_misc.reserve(search ? 16 + lists_bytes : res_bytes)) ||
        (search && (rc = ctx->search_list.reserve(lists_bytes))))
      return rc;
    uint8_t *h_seq = ctx->h_arena.as<uint8_t>();
    uint64_t *h_off_t = ctx->h_desc.as<uint64_t>(), *h_off_q = h_off_t + nt_max;
    uint32_t *h_len_t = reinterpret_cast<uint32_t *>(h_off_q + nq_max), *h_tord = h_len_t + nt_max;
    uint32_t *h_len_q = h_tord + nt_max, *h_qlist = h_len_q + nq_max;
    uint64_t *d_off_t = ctx->off_a.as<uint64_t>(), *d_off_q = d_off_t + nt_max;
    uint32_t *d_len_t = reinterpret_cast<uint32_t *>(d_off_q + nq_max), *d_tord = d_len_t + nt_max;
    uint32_t *d_len_q = d_tord + nt_max, *d_qlist = d_len_q + nq_max;
    uint32_t *d_res = ctx->best_score.as<uint32_t>();
    uint8_t *d_seq = ctx->arena.as<uint8_t>();
    hipStream_t st = ctx->stream;
    const SaFillParams f0 = score_fill_params(sc);

    // sequences idx[first .. first + n) packed from `s` at h_seq + at: offsets (from the device arena's start) and lengths
    auto pack = [&](const seqalign_seqset_t *s, const uint64_t *idx, uint64_t n, uint64_t at, uint64_t *h_off, uint32_t *h_len) {
      uint64_t pos = at;
      for (uint64_t k = 0; k < n; ++k) { h_off[k] = pos; h_len[k] = s->len[idx[k]]; pos += h_len[k]; }
      constexpr uint64_t kTask = 256;
      parallel_for((n + kTask - 1) / kTask, [&](uint64_t blk) {
        for (uint64_t k = blk * kTask, e = std::min(n, (blk + 1) * kTask); k < e; ++k)
          memcpy(h_seq + h_off[k], s->arena + s->off[idx[k]], h_len[k]);
      });
      return pos - at;
    };

    for (const Range &qr : q_ranges) {
      for (const Range &tr : t_ranges) {
        const uint64_t nq = qr.count, nt = tr.count;
        if (t_ranges.size() > 1 || &qr == &q_ranges[0]) {   // the targets of this range (once per call when there is one range)
          const uint64_t bytes = pack(T, ts.data() + tr.first, nt, 0, h_off_t, h_len_t);
          for (uint64_t k = 0; k < nt; ++k) h_tord[k] = (uint32_t)k;
          std::stable_sort(h_tord, h_tord + nt, [&](uint32_t x, uint32_t y) { return h_len_t[x] > h_len_t[y]; });
          if (bytes) HIP_TRY(hipMemcpyAsync(d_seq, h_seq, bytes, hipMemcpyHostToDevice, st));
          HIP_TRY(hipMemcpyAsync(d_off_t, h_off_t, 8 * nt, hipMemcpyHostToDevice, st));
          HIP_TRY(hipMemcpyAsync(d_len_t, h_len_t, 4 * nt, hipMemcpyHostToDevice, st));
          HIP_TRY(hipMemcpyAsync(d_tord, h_tord, 4 * nt, hipMemcpyHostToDevice, st));
        }
        const uint64_t bytes = pack(Q, qs.data() + qr.first, nq, q_at, h_off_q, h_len_q);
        // the queries by row class: q_list holds class 0's, then class 1's, ...
        // (the class past the last, rows for the strips kernel, stays empty: run_short's queries are short; up to
        // SA_SPAN_ROW_MAX columns the span kernels' classes are the score kernels' first SA_SPAN_ROW_CLASSES)
        uint64_t cls_first[SA_SCORE_ROW_CLASSES + 2];
        uint32_t cls_max_a[SA_SCORE_ROW_CLASSES + 1];
        sort_by_row_class(nq, [&](uint64_t k) { return h_len_q[k]; }, h_qlist, cls_first, cls_max_a);
        if (bytes) HIP_TRY(hipMemcpyAsync(d_seq + q_at, h_seq + q_at, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off_q, h_off_q, 8 * nq, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_len_q, h_len_q, 4 * nq, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_qlist, h_qlist, 4 * nq, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_res, 0, 8, st));
        HIP_TRY(hipMemsetAsync(d_res + 2, 0xff, 8, st));
        // search: the query range's lists, laid out for its nq (keys, end_a, end_b, counts), empty at its first target range
        uint8_t *d_lists = ctx->search_list.as<uint8_t>();
        const uint64_t nk = search ? nq * search->k : 0;
        if (search && &tr == &t_ranges.front()) HIP_TRY(hipMemsetAsync(d_lists + 16 * nk, 0, 4 * nq, st));

        const uint64_t n = nq * nt;
        for (int x = 0; x < SA_SCORE_ROW_CLASSES; ++x) {
          const uint64_t m = cls_first[x + 1] - cls_first[x];
          if (!m) continue;
          typename R::CrossParams p;
          memset(&p, 0, sizeof(p));
          p.s.f = f0;
          p.s.f.arena = d_seq;
          p.s.f.off_a = d_off_q; p.s.f.len_a = d_len_q; p.s.f.off_b = d_off_t; p.s.f.len_b = d_len_t;
          p.q_list = d_qlist + cls_first[x]; p.t_order = d_tord;
          p.nq = (uint32_t)m; p.n_t = (uint32_t)nt; p.n_waves = (uint32_t)(m * nt);
          p.s.score = reinterpret_cast<int32_t *>(d_res + 4);
          R::set_results(p.s, d_res + 4, n);
          p.s.err_flag = d_res;
          p.err_pair = reinterpret_cast<unsigned long long *>(d_res + 2);
          const hipError_t e = R::launch_cross(p, cls_max_a[x], is_sw, st);
          if (e != hipSuccess) return fail_hip(e, R::kLaunchCross);
        }

        uint32_t *h = ctx->h_misc.as<uint32_t>();
        if (search) {
          // the rows into the running lists; the error word home, and after the last target range the lists
          SaScoreSelectParams sp;
          memset(&sp, 0, sizeof(sp));
          sp.score = reinterpret_cast<const int32_t *>(d_res + 4);
          if (is_sw) { sp.end_a = d_res + 4 + n; sp.end_b = d_res + 4 + 2 * n; }
          sp.nq = (uint32_t)nq; sp.n_t = (uint32_t)nt; sp.t_base = (uint32_t)tr.first;
          sp.k = search->k; sp.u_max = key_u(search->min_score);
          sp.list_key = reinterpret_cast<unsigned long long *>(d_lists);
          sp.list_ea = reinterpret_cast<uint32_t *>(d_lists + 8 * nk); sp.list_eb = sp.list_ea + nk;
          sp.list_n = sp.list_eb + nk;
          const hipError_t e = sa_launch_score_select(sp, st);
          if (e != hipSuccess) return fail_hip(e, "score select kernel launch");
          const bool last = &tr == &t_ranges.back();
          HIP_TRY(hipMemcpyAsync(h, d_res, 16, hipMemcpyDeviceToHost, st));
          if (last) HIP_TRY(hipMemcpyAsync(h + 4, d_lists, 16 * nk + 4 * nq, hipMemcpyDeviceToHost, st));
          HIP_TRY(stream_wait_spinning(st));
          if (h[0]) {
            uint64_t key;
            memcpy(&key, h + 2, 8);
            fail.offer(qs[qr.first + key / nt], tr.first + key % nt, nT);
          }
          if (!last || fail.any()) continue;
          const uint64_t *hk = reinterpret_cast<const uint64_t *>(h + 4);
          const uint32_t *hea = h + 4 + 2 * nk, *heb = hea + nk, *hn = heb + nk;
          const uint32_t K = search->k;
          for (uint64_t j = 0; j < nq; ++j)
            search->put(qs[qr.first + j], hn[j], hk + j * K, hea + j * K, heb + j * K);
          continue;
        }

        // results home; rows into the matrix
        HIP_TRY(hipMemcpyAsync(h, d_res, 16 + rp * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(stream_wait_spinning(st));
        if (h[0]) {
          uint64_t key;
          memcpy(&key, h + 2, 8);
          fail.offer(qs[qr.first + key / nt], tr.first + key % nt, nT);
          continue;
        }
        if constexpr (R::kMarkField > 0) {   // SA_STATS_NO_WALK in a mismatch word; the tile's order is row-major: its first is its lowest
          const uint32_t *w = h + 4 + (uint64_t)R::kMarkField * n;
          uint64_t k = 0;
          while (k < n && !(w[k] & SA_STATS_NO_WALK)) ++k;
          if (k < n) { no_walk.offer(qs[qr.first + k / nt], tr.first + k % nt, nT); continue; }
        }
        const int32_t *hs = reinterpret_cast<const int32_t *>(h + 4);
        const int nw = fields() - 1;
        constexpr uint64_t kRows = 64;
        parallel_for((nq + kRows - 1) / kRows, [&](uint64_t blk) {
          for (uint64_t k = blk * kRows, e = std::min(nq, (blk + 1) * kRows); k < e; ++k) {
            const uint64_t row = qs[qr.first + k] * nT + tr.first;
            memcpy(out_score + row, hs + k * nt, 4 * nt);
            for (int w = 0; w < nw; ++w) memcpy(out_w[w] + row, h + 4 + (w + 1) * n + k * nt, 4 * nt);
          }
        });
      }
      if (fail.any() || no_walk.any()) break;   // the later query ranges hold only higher pairs
    }
    return SEQALIGN_OK;
  }

  // queries > R::kRowMax: slices of (a few long queries x a slice of the targets) as explicit batches through R's batch call,
  // that is through the strips
  int run_long(const std::vector<uint64_t> &qs) {
    int rc;
    // one arena of their own for the batches: the long queries, then the targets
    std::vector<uint64_t> at_q(qs.size()), at_t(nT);
    uint64_t pos = 0;
    for (uint64_t k = 0; k < qs.size(); ++k) { at_q[k] = pos; pos += Q->len[qs[k]]; }
    for (uint64_t t = 0; t < nT; ++t) { at_t[t] = pos; pos += T->len[t]; }
    std::vector<char> arena(pos + 1);
    for (uint64_t k = 0; k < qs.size(); ++k) memcpy(arena.data() + at_q[k], Q->arena + Q->off[qs[k]], Q->len[qs[k]]);
    for (uint64_t t = 0; t < nT; ++t) memcpy(arena.data() + at_t[t], T->arena + T->off[t], T->len[t]);

    const uint64_t t_slice = std::min(nT, kLongSlicePairs), q_rows = std::max<uint64_t>(1, kLongSlicePairs / nT);
    // search: each long query's best (key, end_a, end_b) so far, cut back to k after every slice
    struct Hit { uint64_t key; uint32_t ea, eb; };
    std::vector<std::vector<Hit>> best(search ? qs.size() : 0);
    const auto by_key = [](const Hit &x, const Hit &y) { return x.key < y.key; };
    std::vector<uint64_t> off_a, off_b;
    std::vector<uint32_t> len_a, len_b, w[6];   // w: the result arrays behind the score (out_w's order)
    std::vector<uint32_t> &ea = w[0], &eb = w[1];
    std::vector<int32_t> sc;
    const int nw = fields() - 1;
    for (uint64_t g0 = 0; g0 < qs.size(); g0 += q_rows) {
      const uint64_t g1 = std::min<uint64_t>(qs.size(), g0 + q_rows);
      if ((fail.any() && qs[g0] > fail.q) || (no_walk.any() && qs[g0] > no_walk.q)) break;   // only higher pairs from here on
      for (uint64_t t0 = 0; t0 < nT; t0 += t_slice) {
        const uint64_t t1 = std::min(nT, t0 + t_slice), nt = t1 - t0, n = (g1 - g0) * nt;
        off_a.resize(n); off_b.resize(n); len_a.resize(n); len_b.resize(n); sc.resize(n);
        for (int x = 0; x < std::max(nw, 2); ++x) w[x].resize(n);
        for (uint64_t k = 0; k < n; ++k) {
          const uint64_t g = g0 + k / nt, t = t0 + k % nt;
          off_a[k] = at_q[g]; len_a[k] = Q->len[qs[g]];
          off_b[k] = at_t[t]; len_b[k] = T->len[t];
        }
        seqalign_batch_t b;
        b.n_pairs = n; b.arena = arena.data(); b.arena_bytes = arena.size();
        b.off_a = off_a.data(); b.len_a = len_a.data(); b.off_b = off_b.data(); b.len_b = len_b.data();
        uint64_t bad = ~0ull;
        uint32_t *const w6[6] = {w[0].data(), w[1].data(), w[2].data(), w[3].data(), w[4].data(), w[5].data()};
        rc = row_batch_call<R>(ctx, &b, scoring, is_sw, sc.data(), w6, &bad);
        if (rc == SEQALIGN_E_TRACEBACK && bad != ~0ull) {
          no_walk.offer(qs[g0 + bad / nt], t0 + bad % nt, nT);
          continue;
        }
        if (rc == SEQALIGN_E_UNKNOWN_PAIR && bad != ~0ull) {
          fail.offer(qs[g0 + bad / nt], t0 + bad % nt, nT);
          continue;
        }
        if (rc) return rc;
        if (search) {
          for (uint64_t k = 0; k < n; ++k)
            if (sc[k] >= search->min_score) best[g0 + k / nt].push_back({hit_key(sc[k], t0 + k % nt), ea[k], eb[k]});
          for (uint64_t g = g0; g < g1; ++g) {
            std::vector<Hit> &b = best[g];
            if (b.size() <= search->k) continue;
            std::nth_element(b.begin(), b.begin() + search->k, b.end(), by_key);
            b.resize(search->k);
          }
          continue;
        }
        for (uint64_t k = 0; k < n; ++k) {
          const uint64_t at = qs[g0 + k / nt] * nT + t0 + k % nt;
          out_score[at] = sc[k];
          for (int x = 0; x < nw; ++x) out_w[x][at] = w[x][k];
        }
      }
      if (fail.any()) break;
    }
    if (search && !fail.any()) {
      std::vector<uint64_t> key;
      std::vector<uint32_t> ea_, eb_;
      for (uint64_t g = 0; g < qs.size(); ++g) {
        std::vector<Hit> &b = best[g];
        std::sort(b.begin(), b.end(), by_key);
        key.resize(b.size()); ea_.resize(b.size()); eb_.resize(b.size());
        for (size_t i = 0; i < b.size(); ++i) { key[i] = b[i].key; ea_[i] = b[i].ea; eb_[i] = b[i].eb; }
        search->put(qs[g], (uint32_t)b.size(), key.data(), ea_.data(), eb_.data());
      }
    }
    return SEQALIGN_OK;
  }

  // both paths, then the failing pair's message -- q_base: what the message adds to a query index (the *_multi calls)
  int run(uint64_t q_base) {
    int rc;
    std::vector<uint64_t> short_q, long_q;
    {   // the scoring's int32 domain over the longest query and the longest target, before anything is launched
      seqalign_dev_scoring *sc = nullptr;
      if ((rc = cached_scoring(ctx, scoring, is_sw ? 1 : 0, &sc))) return rc;
      uint32_t max_q = 0, max_t = 0;
      for (uint64_t q = 0; q < Q->n_seqs; ++q) max_q = std::max(max_q, Q->len[q]);
      for (uint64_t t = 0; t < T->n_seqs; ++t) max_t = std::max(max_t, T->len[t]);
      if ((rc = admit_magnitude(sc, max_q, max_t, SA_FRAMES_ROWS))) return rc;
    }
    for (uint64_t q = 0; q < Q->n_seqs; ++q) (Q->len[q] > R::kRowMax ? long_q : short_q).push_back(q);
    if (!short_q.empty() && (rc = run_short(short_q))) return rc;
    if (!long_q.empty() && (rc = run_long(long_q))) return rc;
    if (no_walk.any() && no_walk.key < fail.key) {   // the lowest failing pair's code is the call's
      set_last_error("query " + std::to_string(q_base + no_walk.q) + ", target " + std::to_string(no_walk.t) + ": traceback failed");
      return SEQALIGN_E_TRACEBACK;
    }
    if (fail.any()) {
      set_last_error("query " + std::to_string(q_base + fail.q) + ", target " + std::to_string(fail.t) +
                     ": a character pair without a score");
      return SEQALIGN_E_UNKNOWN_PAIR;
    }
    return SEQALIGN_OK;
  }
};

int check_set(const seqalign_seqset_t *s) {
  return !s || (s->n_seqs && (!s->arena || !s->off || !s->len)) ? SEQALIGN_E_ARG : SEQALIGN_OK;
}

}  // namespace

int sa_host::score_cross_check(const seqalign_seqset_t *queries, const seqalign_seqset_t *targets) {
  if (check_set(queries) || check_set(targets)) return SEQALIGN_E_ARG;
  if (targets->n_seqs && queries->n_seqs > ~0ull / targets->n_seqs) {
    set_last_error("score cross: n_queries x n_targets overflows 64 bits");
    return SEQALIGN_E_ARG;
  }
  return SEQALIGN_OK;
}

template <class R>
int sa_host::cross_call(const CrossArgs &a) {
  CallScope scope(a.ctx);
  if (!a.queries->n_seqs || !a.targets->n_seqs) return SEQALIGN_OK;
  HIP_TRY(hipSetDevice(a.ctx->device));
  StreamSyncOnExit sync(a.ctx->stream);
  CrossCall<R> call{.ctx = a.ctx, .Q = a.queries, .T = a.targets, .scoring = a.scoring, .is_sw = a.is_sw,
                    .out_score = a.out_score, .out_w = a.out_w, .nT = a.targets->n_seqs};
  return call.run(a.q_base);
}
template int sa_host::cross_call<ScoreTraits>(const CrossArgs &);
template int sa_host::cross_call<SpanTraits>(const CrossArgs &);
template int sa_host::cross_call<StatsTraits>(const CrossArgs &);
template int sa_host::cross_call<SwStatsTraits>(const CrossArgs &);
template int sa_host::cross_call<NwGapsTraits>(const CrossArgs &);

int sa_host::score_search_check(const seqalign_seqset_t *queries, const seqalign_seqset_t *targets, uint32_t k) {
  if (k == 0 || k > SEQALIGN_SEARCH_MAX_K) {
    set_last_error("score search: k must be 1 .. " + std::to_string(SEQALIGN_SEARCH_MAX_K));
    return SEQALIGN_E_ARG;
  }
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  if (targets->n_seqs > UINT32_MAX) {
    set_last_error("score search: more than UINT32_MAX targets");
    return SEQALIGN_E_ARG;
  }
  return SEQALIGN_OK;
}

int sa_host::score_search_call(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                               const scoring_t *scoring, bool is_sw, uint32_t k, int32_t min_score,
                               seqalign_search_hit_t *hits, uint32_t *n_hits, uint64_t q_base) {
  int rc = score_search_check(queries, targets, k);
  if (rc) return rc;
  CallScope scope(ctx);
  if (!queries->n_seqs) return SEQALIGN_OK;
  if (!targets->n_seqs) {
    memset(n_hits, 0, 4 * queries->n_seqs);
    return SEQALIGN_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  StreamSyncOnExit sync(ctx->stream);
  const SearchOut out{k, min_score, hits, n_hits};
  CrossCall<ScoreTraits> call{.ctx = ctx, .Q = queries, .T = targets, .scoring = scoring, .is_sw = is_sw,
                              .out_score = nullptr, .out_w = nullptr, .nT = targets->n_seqs, .search = &out};
  return call.run(q_base);
}

namespace {

// seqalign_sw_span_search's second stage.  `hits` holds the first stage's lists with len_a / len_b = the best cell (end_a,
// end_b) and pos 0.  Every hit above 0 becomes one pair of an explicit list: query[0 : end_a] against target[0 : end_b], whose
// first hit is the full pair's in all five fields -- and whose row is as short as the hit allows.  What is
// built here grows with the hits: each query that has one is copied once, up to its furthest end, and each hit's target prefix.
int span_of_hits(seqalign_ctx_t *ctx, const seqalign_seqset_t *Q, const seqalign_seqset_t *T, const scoring_t *scoring, uint32_t k,
                 seqalign_span_hit_t *hits, const uint32_t *n_hits, uint64_t q_base) {
  uint64_t n = 0, bytes = 0;
  for (uint64_t q = 0; q < Q->n_seqs; ++q) {
    uint32_t q_end = 0;
    for (uint32_t i = 0; i < n_hits[q]; ++i) {
      const seqalign_span_hit_t &h = hits[q * k + i];
      if (h.score <= 0) continue;
      n++; bytes += h.len_b; q_end = std::max(q_end, h.len_a);
    }
    bytes += q_end;
  }
  if (!n) return SEQALIGN_OK;   // (hits of score 0 hold five zeros already)
  std::vector<char> arena(bytes + 1);
  std::vector<uint64_t> off_a(n), off_b(n), where(n);
  std::vector<uint32_t> len_a(n), len_b(n), res(4 * n);
  std::vector<int32_t> sc(n);
  uint64_t at = 0, pos = 0;
  for (uint64_t q = 0; q < Q->n_seqs; ++q) {
    const uint64_t q_at = pos, first = at;
    uint32_t q_end = 0;
    for (uint32_t i = 0; i < n_hits[q]; ++i) {
      const seqalign_span_hit_t &h = hits[q * k + i];
      if (h.score <= 0) continue;
      where[at] = q * k + i;
      len_a[at] = h.len_a; len_b[at] = h.len_b;
      q_end = std::max(q_end, h.len_a);
      ++at;
    }
    memcpy(arena.data() + q_at, Q->arena + Q->off[q], q_end);
    pos += q_end;
    for (uint64_t j = first; j < at; ++j) {
      off_a[j] = q_at; off_b[j] = pos;
      memcpy(arena.data() + pos, T->arena + T->off[hits[where[j]].target], len_b[j]);
      pos += len_b[j];
    }
  }
  seqalign_batch_t b;
  b.n_pairs = n; b.arena = arena.data(); b.arena_bytes = arena.size();
  b.off_a = off_a.data(); b.len_a = len_a.data(); b.off_b = off_b.data(); b.len_b = len_b.data();
  uint64_t bad = ~0ull;
  const int rc = span_batch_impl(ctx, &b, scoring, sc.data(), res.data(), res.data() + n, res.data() + 2 * n, res.data() + 3 * n, &bad);
  if (rc == SEQALIGN_E_UNKNOWN_PAIR && bad != ~0ull)   // (the first stage swept these cells and found none: kept for the message)
    set_last_error("query " + std::to_string(q_base + where[bad] / k) + ", target " + std::to_string(hits[where[bad]].target) +
                   ": a character pair without a score");
  if (rc) return rc;
  for (uint64_t j = 0; j < n; ++j) {
    seqalign_span_hit_t &h = hits[where[j]];
    h.pos_a = res[j]; h.pos_b = res[n + j]; h.len_a = res[2 * n + j]; h.len_b = res[3 * n + j];
  }
  return SEQALIGN_OK;
}

}  // namespace

int sa_host::span_search_call(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                              const scoring_t *scoring, uint32_t k, int32_t min_score, seqalign_span_hit_t *hits,
                              uint32_t *n_hits, uint64_t q_base) {
  int rc = score_search_check(queries, targets, k);
  if (rc) return rc;
  CallScope scope(ctx);
  if (!queries->n_seqs) return SEQALIGN_OK;
  if (!targets->n_seqs) {
    memset(n_hits, 0, 4 * queries->n_seqs);
    return SEQALIGN_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  StreamSyncOnExit sync(ctx->stream);
  const SearchOut out{k, min_score, nullptr, n_hits, hits};
  CrossCall<ScoreTraits> call{.ctx = ctx, .Q = queries, .T = targets, .scoring = scoring, .is_sw = true,
                              .out_score = nullptr, .out_w = nullptr, .nT = targets->n_seqs, .search = &out};
  if ((rc = call.run(q_base))) return rc;
  return span_of_hits(ctx, queries, targets, scoring, k, hits, n_hits, q_base);
}

extern "C" int seqalign_nw_score_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                       const scoring_t *scoring, int32_t *out_score) {
  if (!ctx || !scoring || !out_score) return SEQALIGN_E_ARG;
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  return cross_call<ScoreTraits>({.ctx = ctx, .queries = queries, .targets = targets, .scoring = scoring,
                                  .is_sw = false, .out_score = out_score, .out_w = nullptr, .q_base = 0});
}

extern "C" int seqalign_sw_score_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                       const scoring_t *scoring, int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b) {
  if (!ctx || !scoring || !out_score || !out_end_a || !out_end_b) return SEQALIGN_E_ARG;
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  uint32_t *const out_w[2] = {out_end_a, out_end_b};
  return cross_call<ScoreTraits>({.ctx = ctx, .queries = queries, .targets = targets, .scoring = scoring,
                                  .is_sw = true, .out_score = out_score, .out_w = out_w, .q_base = 0});
}

extern "C" int seqalign_nw_score_search(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                        const scoring_t *scoring, uint32_t k, int32_t min_score, seqalign_search_hit_t *hits,
                                        uint32_t *n_hits) {
  if (!ctx || !scoring || !hits || !n_hits) return SEQALIGN_E_ARG;
  return score_search_call(ctx, queries, targets, scoring, false, k, min_score, hits, n_hits, 0);
}

extern "C" int seqalign_sw_score_search(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                        const scoring_t *scoring, uint32_t k, int32_t min_score, seqalign_search_hit_t *hits,
                                        uint32_t *n_hits) {
  if (!ctx || !scoring || !hits || !n_hits) return SEQALIGN_E_ARG;
  return score_search_call(ctx, queries, targets, scoring, true, k, min_score, hits, n_hits, 0);
}

extern "C" int seqalign_sw_span_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                      const scoring_t *scoring, int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b,
                                      uint32_t *out_len_a, uint32_t *out_len_b) {
  if (!ctx || !scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b) return SEQALIGN_E_ARG;
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  uint32_t *const out_w[4] = {out_pos_a, out_pos_b, out_len_a, out_len_b};
  return cross_call<SpanTraits>({.ctx = ctx, .queries = queries, .targets = targets, .scoring = scoring,
                                 .is_sw = true, .out_score = out_score, .out_w = out_w, .q_base = 0});
}

extern "C" int seqalign_sw_span_search(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                       const scoring_t *scoring, uint32_t k, int32_t min_score, seqalign_span_hit_t *hits,
                                       uint32_t *n_hits) {
  if (!ctx || !scoring || !hits || !n_hits) return SEQALIGN_E_ARG;
  return span_search_call(ctx, queries, targets, scoring, k, min_score, hits, n_hits, 0);
}

extern "C" int seqalign_nw_stats_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                       const scoring_t *scoring, int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches) {
  if (!ctx || !scoring || !out_score || !out_matches || !out_mismatches) return SEQALIGN_E_ARG;
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  uint32_t *const out_w[2] = {out_matches, out_mismatches};
  return cross_call<StatsTraits>({.ctx = ctx, .queries = queries, .targets = targets, .scoring = scoring,
                                  .is_sw = false, .out_score = out_score, .out_w = out_w, .q_base = 0});
}

// NW gap-run matrices: seqalign_nw_stats_cross with the gap-run kernels
extern "C" int seqalign_nw_gaps_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                      const scoring_t *scoring, int32_t *out_score, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b) {
  if (!ctx || !scoring || !out_score || !out_gap_runs_a || !out_gap_runs_b) return SEQALIGN_E_ARG;
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  uint32_t *const out_w[2] = {out_gap_runs_a, out_gap_runs_b};
  return cross_call<NwGapsTraits>({.ctx = ctx, .queries = queries, .targets = targets, .scoring = scoring,
                                   .is_sw = false, .out_score = out_score, .out_w = out_w, .q_base = 0});
}

// seqalign_sw_stats_*'s length limit over a set (sa_host::sw_stats_check_batch): the lowest sequence over it is named
static int sw_stats_check_set(const seqalign_seqset_t *s, const char *what) {
  for (uint64_t i = 0; i < s->n_seqs; ++i)
    if (s->len[i] > SEQALIGN_SW_STATS_MAX_LEN) {
      set_last_error(std::string(what) + " " + std::to_string(i) + ": " + std::to_string(s->len[i]) +
                     " letters, SW statistics take at most " + std::to_string(SEQALIGN_SW_STATS_MAX_LEN));
      return SEQALIGN_E_TOO_LARGE;
    }
  return SEQALIGN_OK;
}

extern "C" int seqalign_sw_stats_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                                       const scoring_t *scoring, int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b,
                                       uint32_t *out_len_a, uint32_t *out_len_b, uint32_t *out_matches, uint32_t *out_mismatches) {
  if (!scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b || !out_matches || !out_mismatches)
    return SEQALIGN_E_ARG;
  int rc = score_cross_check(queries, targets);
  if (rc || (rc = sw_stats_check_set(queries, "query")) || (rc = sw_stats_check_set(targets, "target"))) return rc;
  if (!ctx) return SEQALIGN_E_ARG;   // (the limit is the arguments' own: found before the context is looked at)
  uint32_t *const out_w[6] = {out_pos_a, out_pos_b, out_len_a, out_len_b, out_matches, out_mismatches};
  return cross_call<SwStatsTraits>({.ctx = ctx, .queries = queries, .targets = targets, .scoring = scoring,
                                    .is_sw = true, .out_score = out_score, .out_w = out_w, .q_base = 0});
}
