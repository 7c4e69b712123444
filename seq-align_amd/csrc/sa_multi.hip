// sa_multi.hip -- the host-level calls over several contexts (GPUs) from one process.
#include "sa_row_families.hpp"

using namespace sa_host;

// ------------------------------------------------- several contexts (GPUs) ---
namespace {

// pairs [first, first + count) of a batch as a batch of their own (views, nothing copied)
seqalign_batch_t sub_batch(const seqalign_batch_t *b, uint64_t first, uint64_t count) {
  seqalign_batch_t s = *b;
  s.n_pairs = count;
  s.off_a = b->off_a + first; s.len_a = b->len_a + first;
  s.off_b = b->off_b + first; s.len_b = b->len_b + first;
  return s;
}

// n_ctx + 1 pair indices cutting the batch into contiguous ranges of (nearly) equal DP cells
// (balance ragged batches by W*H; contiguous, so results stay in pair order): edge k is the
// pair boundary nearest to k/n_ctx of the cell total, ties to the later boundary -- the rule of
// workloads.shard_edges_cells on the Python side.
std::vector<uint64_t> shard_edges_cum(const std::vector<uint64_t> &cum, int n_ctx) {   // cum[k]: cells of items 0 .. k - 1
  const uint64_t n = cum.size() - 1;
  const uint64_t total = cum[n];
  std::vector<uint64_t> edges((size_t)n_ctx + 1, 0);
  for (int k = 1; k < n_ctx; ++k) {
    const uint64_t t = (uint64_t)(((unsigned __int128)total * (unsigned)k) / (unsigned)n_ctx);
    uint64_t i = (uint64_t)(std::lower_bound(cum.begin(), cum.end(), t) - cum.begin());
    if (i > n) i = n;
    if (i > 0 && t - cum[i - 1] < cum[i] - t) --i;
    edges[k] = std::max(i, edges[k - 1]);
  }
  edges[n_ctx] = n;
  return edges;
}

std::vector<uint64_t> shard_edges(const seqalign_batch_t *b, int n_ctx) {
  const uint64_t n = b->n_pairs;
  std::vector<uint64_t> cum(n + 1, 0);
  for (uint64_t p = 0; p < n; ++p) cum[p + 1] = cum[p] + (uint64_t)(b->len_a[p] + 1ull) * (b->len_b[p] + 1ull);
  return shard_edges_cum(cum, n_ctx);
}

// run fn(g, first, count) for the n_ctx contiguous ranges, one host thread each; first error wins
template <class F>
int for_each_shard(const std::vector<uint64_t> &edges, F fn) {
  const int n_ctx = (int)edges.size() - 1;
  std::vector<int> rc((size_t)n_ctx, SEQALIGN_OK);
  std::vector<std::string> msg((size_t)n_ctx);
  std::vector<std::thread> th;
  for (int g = 0; g < n_ctx; ++g) {
    const uint64_t first = edges[g], last = edges[g + 1];
    th.emplace_back([&, g, first, last] {
      rc[g] = last > first ? fn(g, first, last - first) : SEQALIGN_OK;
      if (rc[g]) msg[g] = seqalign_last_error();   // the message lives in the worker's thread
    });
  }
  for (auto &t : th) t.join();
  for (int g = 0; g < n_ctx; ++g)
    if (rc[g]) { set_last_error(msg[g]); return rc[g]; }
  return SEQALIGN_OK;
}

bool bad_ctx_list(seqalign_ctx_t *const *ctxs, int n_ctx) {
  if (!ctxs || n_ctx <= 0) return true;
  for (int g = 0; g < n_ctx; ++g)
    if (!ctxs[g]) return true;
  return false;
}

}  // namespace

extern "C" int seqalign_fill_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                         const scoring_t *scoring, int is_sw, const uint64_t *mat_off,
                                         int32_t *match_scores, int32_t *gap_a_scores, int32_t *gap_b_scores,
                                         uint64_t *status) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch || !mat_off) return SEQALIGN_E_ARG;
  int rc = check_batch(batch);
  if (rc) return rc;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);   // mat_off[] are absolute cell offsets: shared arenas
    return seqalign_fill_batch(ctxs[g], &s, scoring, is_sw, mat_off + first, match_scores, gap_a_scores, gap_b_scores,
                               status ? status + first : nullptr);
  });
}

extern "C" int seqalign_nw_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                       const scoring_t *scoring, const uint64_t *str_off, char *out_a, char *out_b,
                                       uint32_t *out_len, int32_t *out_score) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch || !str_off || !out_len || !out_score) return SEQALIGN_E_ARG;
  int rc = check_batch(batch);
  if (rc) return rc;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);   // str_off[] are absolute: shared string buffers
    return seqalign_nw_batch(ctxs[g], &s, scoring, str_off + first, out_a, out_b, out_len + first, out_score + first);
  });
}

extern "C" int seqalign_nw_batch_cigar_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                             const scoring_t *scoring, int format, const uint64_t *cigar_off, char *cigar,
                                             uint32_t *cigar_len, int32_t *out_score) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch || !cigar_off || !cigar || !cigar_len || !out_score) return SEQALIGN_E_ARG;
  int rc = check_batch(batch);
  if (rc) return rc;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);   // cigar_off[] are absolute: one shared buffer
    return seqalign_nw_batch_cigar(ctxs[g], &s, scoring, format, cigar_off + first, cigar, cigar_len + first, out_score + first);
  });
}

// format 0: the two strings (seqalign_sw_batch_multi); 1 / 2: CIGAR (seqalign_sw_batch_cigar_multi; out_b unused)
static int sw_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                          const scoring_t *scoring, const int32_t *min_score, uint32_t max_hits, int format,
                          seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits, char *out_a,
                          char *out_b, uint64_t str_cap) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch || !min_score || !hits || !n_hits || !out_a || (!format && !out_b)) return SEQALIGN_E_ARG;
  *n_hits = 0;
  int rc = check_batch(batch);
  if (rc) return rc;
  const uint64_t n = batch->n_pairs;
  if (n == 0) return SEQALIGN_OK;
  // every range writes into its own slice of the caller's buffers; the slices are closed up afterwards
  std::vector<uint64_t> h0((size_t)n_ctx + 1), s0((size_t)n_ctx + 1), got((size_t)n_ctx, 0), used((size_t)n_ctx, 0);
  const std::vector<uint64_t> edges = shard_edges(batch, n_ctx);
  for (int g = 0; g <= n_ctx; ++g) {
    const uint64_t first = edges[g];
    h0[g] = (uint64_t)((long double)hit_cap * first / n);
    s0[g] = (uint64_t)((long double)str_cap * first / n);
  }
  rc = for_each_shard(edges, [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);
    uint64_t found = 0;
    const int r = format ? seqalign_sw_batch_cigar(ctxs[g], &s, scoring, min_score + first, max_hits, format, hits + h0[g], h0[g + 1] - h0[g],
                                                   &found, out_a + s0[g], s0[g + 1] - s0[g])
                         : seqalign_sw_batch(ctxs[g], &s, scoring, min_score + first, max_hits, hits + h0[g], h0[g + 1] - h0[g],
                                             &found, out_a + s0[g], out_b + s0[g], s0[g + 1] - s0[g]);
    got[g] = found;
    for (uint64_t i = 0; i < found; ++i) {
      const seqalign_sw_hit_t &h = hits[h0[g] + i];
      // (a hit's text: its columns, or in CIGAR mode the CIGAR -- the hits lie back to back, so only the last one's end matters)
      used[g] = std::max(used[g], h.str_off + (format ? strlen(out_a + s0[g] + h.str_off) : (size_t)h.length) + 1);
    }
    return r;
  });
  if (rc) return rc;
  uint64_t nh = 0, ns = 0;
  for (int g = 0; g < n_ctx; ++g) {
    const uint64_t first = edges[g];
    if (s0[g] != ns) {
      memmove(out_a + ns, out_a + s0[g], used[g]);
      if (!format) memmove(out_b + ns, out_b + s0[g], used[g]);
    }
    for (uint64_t i = 0; i < got[g]; ++i) {
      seqalign_sw_hit_t h = hits[h0[g] + i];
      h.pair += first;            // range-relative -> batch index
      h.str_off += ns;            // slice-relative -> buffer offset
      hits[nh++] = h;
    }
    ns += used[g];
  }
  *n_hits = nh;
  return SEQALIGN_OK;
}

extern "C" int seqalign_sw_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                       const scoring_t *scoring, const int32_t *min_score, uint32_t max_hits,
                                       seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits, char *out_a,
                                       char *out_b, uint64_t str_cap) {
  return sw_batch_multi(ctxs, n_ctx, batch, scoring, min_score, max_hits, 0, hits, hit_cap, n_hits, out_a, out_b, str_cap);
}

extern "C" int seqalign_sw_batch_cigar_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                             const scoring_t *scoring, const int32_t *min_score, uint32_t max_hits, int format,
                                             seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits, char *cigar,
                                             uint64_t cigar_cap) {
  if (format != SEQALIGN_CIGAR_M && format != SEQALIGN_CIGAR_EQX) return SEQALIGN_E_ARG;
  return sw_batch_multi(ctxs, n_ctx, batch, scoring, min_score, max_hits, format, hits, hit_cap, n_hits, cigar, nullptr, cigar_cap);
}

// score only: the same contiguous ranges; every range writes its own slice of the per-pair outputs
extern "C" int seqalign_nw_score_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                             const scoring_t *scoring, int32_t *out_score) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch_readable(batch) || !scoring || !out_score) return SEQALIGN_E_ARG;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);
    return seqalign_nw_score_batch(ctxs[g], &s, scoring, out_score + first);
  });
}

extern "C" int seqalign_sw_score_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                             const scoring_t *scoring, int32_t *out_score, uint32_t *out_end_a,
                                             uint32_t *out_end_b) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch_readable(batch) || !scoring || !out_score || !out_end_a || !out_end_b) return SEQALIGN_E_ARG;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);
    return seqalign_sw_score_batch(ctxs[g], &s, scoring, out_score + first, out_end_a + first, out_end_b + first);
  });
}

extern "C" int seqalign_sw_span_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                            const scoring_t *scoring, int32_t *out_score, uint32_t *out_pos_a,
                                            uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch_readable(batch) || !scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a ||
      !out_len_b)
    return SEQALIGN_E_ARG;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);
    return seqalign_sw_span_batch(ctxs[g], &s, scoring, out_score + first, out_pos_a + first, out_pos_b + first,
                                  out_len_a + first, out_len_b + first);
  });
}

extern "C" int seqalign_nw_stats_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                             const scoring_t *scoring, int32_t *out_score, uint32_t *out_matches,
                                             uint32_t *out_mismatches) {
  if (bad_ctx_list(ctxs, n_ctx) || !batch_readable(batch) || !scoring || !out_score || !out_matches || !out_mismatches)
    return SEQALIGN_E_ARG;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);
    return seqalign_nw_stats_batch(ctxs[g], &s, scoring, out_score + first, out_matches + first, out_mismatches + first);
  });
}

extern "C" int seqalign_sw_stats_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                             const scoring_t *scoring, int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b,
                                             uint32_t *out_len_a, uint32_t *out_len_b, uint32_t *out_matches,
                                             uint32_t *out_mismatches) {
  if (!ctxs || n_ctx <= 0 || !batch_readable(batch) || !scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b ||
      !out_matches || !out_mismatches)
    return SEQALIGN_E_ARG;
  int rc = sw_stats_check_batch(batch);   // (the whole batch's pair index, before any context is looked at)
  if (rc) return rc;
  if (bad_ctx_list(ctxs, n_ctx)) return SEQALIGN_E_ARG;
  return for_each_shard(shard_edges(batch, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    const seqalign_batch_t s = sub_batch(batch, first, count);
    return seqalign_sw_stats_batch(ctxs[g], &s, scoring, out_score + first, out_pos_a + first, out_pos_b + first, out_len_a + first,
                                   out_len_b + first, out_matches + first, out_mismatches + first);
  });
}

// score matrices: contiguous query ranges of nearly equal cells -- a query's cells are (len + 1) x the targets' sum of
// (len + 1), a factor common to all, so the ranges are cut by len + 1 -- each context writes its own rows
namespace {
// fn(g, the range's queries as a set of their own, first) for the n_ctx query ranges
template <class F>
int for_each_query_shard(const seqalign_seqset_t *queries, int n_ctx, F fn) {
  const uint64_t nq = queries->n_seqs;
  std::vector<uint64_t> cum(nq + 1, 0);
  for (uint64_t q = 0; q < nq; ++q) cum[q + 1] = cum[q] + queries->len[q] + 1ull;
  return for_each_shard(shard_edges_cum(cum, n_ctx), [&](int g, uint64_t first, uint64_t count) {
    seqalign_seqset_t s = *queries;
    s.n_seqs = count; s.off = queries->off + first; s.len = queries->len + first;
    return fn(g, &s, first);
  });
}

int score_cross_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                      const scoring_t *scoring, bool is_sw, int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b) {
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  const uint64_t nq = queries->n_seqs, nt = targets->n_seqs;
  if (!nq || !nt) return SEQALIGN_OK;
  return for_each_query_shard(queries, n_ctx, [&](int g, const seqalign_seqset_t *s, uint64_t first) {
    uint32_t *const out_w[2] = {is_sw ? out_end_a + first * nt : nullptr, is_sw ? out_end_b + first * nt : nullptr};
    return cross_call<ScoreTraits>({.ctx = ctxs[g], .queries = s, .targets = targets, .scoring = scoring,
                                    .is_sw = is_sw, .out_score = out_score + first * nt, .out_w = out_w, .q_base = first});
  });
}
}  // namespace

extern "C" int seqalign_nw_score_cross_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                             const seqalign_seqset_t *targets, const scoring_t *scoring, int32_t *out_score) {
  if (bad_ctx_list(ctxs, n_ctx) || !scoring || !out_score) return SEQALIGN_E_ARG;
  return score_cross_multi(ctxs, n_ctx, queries, targets, scoring, false, out_score, nullptr, nullptr);
}

extern "C" int seqalign_sw_score_cross_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                             const seqalign_seqset_t *targets, const scoring_t *scoring, int32_t *out_score,
                                             uint32_t *out_end_a, uint32_t *out_end_b) {
  if (bad_ctx_list(ctxs, n_ctx) || !scoring || !out_score || !out_end_a || !out_end_b) return SEQALIGN_E_ARG;
  return score_cross_multi(ctxs, n_ctx, queries, targets, scoring, true, out_score, out_end_a, out_end_b);
}

// top-k search: the query ranges of score_cross_multi, each context writes its queries' lists and counts
namespace {
int score_search_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                       const scoring_t *scoring, bool is_sw, uint32_t k, int32_t min_score, seqalign_search_hit_t *hits,
                       uint32_t *n_hits) {
  int rc = score_search_check(queries, targets, k);
  if (rc) return rc;
  if (!queries->n_seqs) return SEQALIGN_OK;
  return for_each_query_shard(queries, n_ctx, [&](int g, const seqalign_seqset_t *s, uint64_t first) {
    return score_search_call(ctxs[g], s, targets, scoring, is_sw, k, min_score, hits + first * k, n_hits + first, first);
  });
}
}  // namespace

extern "C" int seqalign_nw_score_search_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                              const seqalign_seqset_t *targets, const scoring_t *scoring, uint32_t k,
                                              int32_t min_score, seqalign_search_hit_t *hits, uint32_t *n_hits) {
  if (bad_ctx_list(ctxs, n_ctx) || !scoring || !hits || !n_hits) return SEQALIGN_E_ARG;
  return score_search_multi(ctxs, n_ctx, queries, targets, scoring, false, k, min_score, hits, n_hits);
}

extern "C" int seqalign_sw_score_search_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                              const seqalign_seqset_t *targets, const scoring_t *scoring, uint32_t k,
                                              int32_t min_score, seqalign_search_hit_t *hits, uint32_t *n_hits) {
  if (bad_ctx_list(ctxs, n_ctx) || !scoring || !hits || !n_hits) return SEQALIGN_E_ARG;
  return score_search_multi(ctxs, n_ctx, queries, targets, scoring, true, k, min_score, hits, n_hits);
}

// span matrices and the search with spans: the query ranges of the score forms
extern "C" int seqalign_sw_span_cross_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                            const seqalign_seqset_t *targets, const scoring_t *scoring, int32_t *out_score,
                                            uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b) {
  if (bad_ctx_list(ctxs, n_ctx) || !scoring || !out_score || !out_pos_a || !out_pos_b || !out_len_a || !out_len_b) return SEQALIGN_E_ARG;
  int rc = score_cross_check(queries, targets);
  if (rc) return rc;
  const uint64_t nt = targets->n_seqs;
  if (!queries->n_seqs || !nt) return SEQALIGN_OK;
  return for_each_query_shard(queries, n_ctx, [&](int g, const seqalign_seqset_t *s, uint64_t first) {
    uint32_t *const out_w[4] = {out_pos_a + first * nt, out_pos_b + first * nt, out_len_a + first * nt, out_len_b + first * nt};
    return cross_call<SpanTraits>({.ctx = ctxs[g], .queries = s, .targets = targets, .scoring = scoring,
                                   .is_sw = true, .out_score = out_score + first * nt, .out_w = out_w, .q_base = first});
  });
}

extern "C" int seqalign_sw_span_search_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                             const seqalign_seqset_t *targets, const scoring_t *scoring, uint32_t k,
                                             int32_t min_score, seqalign_span_hit_t *hits, uint32_t *n_hits) {
  if (bad_ctx_list(ctxs, n_ctx) || !scoring || !hits || !n_hits) return SEQALIGN_E_ARG;
  int rc = score_search_check(queries, targets, k);
  if (rc) return rc;
  if (!queries->n_seqs) return SEQALIGN_OK;
  return for_each_query_shard(queries, n_ctx, [&](int g, const seqalign_seqset_t *s, uint64_t first) {
    return span_search_call(ctxs[g], s, targets, scoring, k, min_score, hits + first * k, n_hits + first, first);
  });
}
