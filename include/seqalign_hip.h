/*
 * seqalign_hip.h -- C ABI of the MI355X (gfx950) DP-fill engine.
 *
 * This is the drop-in boundary for the ONE hot path of noporpoise/seq-align:
 * the O(n*m) affine-gap fill of the match / gap_a / gap_b score matrices
 * (reference: static alignment_fill_matrices, src/alignment.c:28-168, reached
 * only through aligner_align, src/alignment.c:170-193).  Plain pointers and
 * sizes only; no C++ or torch types.  Built by seq-align_amd/Makefile into
 * seq-align_amd/lib/libseqalign_hip.so together with the host-side mirror of the
 * reference API (alignment.h, alignment_scoring.h, needleman_wunsch.h,
 * smith_waterman.h in this directory).
 *
 * The reference aligns one pair per call (callback per pair,
 * src/alignment_cmdline.c:611-622); a 150x150 fill is ~23 k cells, far below one
 * kernel launch, so the new surface here is a BATCH of independent pairs.
 * aligner_align() itself is kept (alignment.h) and is a batch of one.
 *
 * There is NO CPU fallback: every entry point that needs the device fails with
 * SEQALIGN_E_NO_DEVICE / SEQALIGN_E_HIP when the HIP runtime or a gfx950 device
 * is missing.
 *
 * Output contract (bit-exact with the reference): for pair p the three matrices
 * hold (len_a+1)*(len_b+1) int32 each, dense pitch W=len_a+1, cell (i,j) at
 * j*W+i (ARR_2D_INDEX, src/alignment_macros.h:11), starting mat_off[p] cells
 * into each of the three arenas.
 */
#ifndef SEQALIGN_HIP_H
#define SEQALIGN_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "seqalign_compat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------- */
enum {
  SEQALIGN_OK = 0,
  SEQALIGN_E_NO_DEVICE = 1,   /* no HIP runtime / no gfx950 device            */
  SEQALIGN_E_HIP = 2,         /* a HIP call failed (see seqalign_last_error)  */
  SEQALIGN_E_ARG = 3,         /* bad argument                                 */
  SEQALIGN_E_NOMEM = 4,
  SEQALIGN_E_UNKNOWN_PAIR = 5,/* character pair without a score and
                                 use_match_mismatch==0; the reference exit()s
                                 here (src/alignment_scoring.c:178-181)       */
  SEQALIGN_E_DOMAIN = 6,      /* NW scoring whose gap penalties are below
                                 -|min_penalty|: signed overflow (UB) in the
                                 reference fill; or scores too
                                 large for the row sweeps (below)              */
  SEQALIGN_E_TRACEBACK = 7,   /* src/alignment.c:328-349 would exit()         */
  SEQALIGN_E_TOO_LARGE = 8    /* one pair needs >= 2^31 cells                 */
};

/* SEQALIGN_E_DOMAIN, the second case.  The kernels de-trend gap_b along a row: they add to a cell up to `cols` times
 * |gap_extend| before they take a maximum, a sum the reference never forms, and it must fit int32.  With la / lb the longest
 * seq_a / seq_b of the call (score_cross, score_search: the longest query / target) and n = min(la, lb), no cell holds more than
 *     bound = max(n P + (la + lb - 2 n) G, (la + lb) G)
 * P = the largest substitution score above 0 (match, mismatch, every table entry), G = the largest of gap_open + gap_extend and
 * gap_extend above 0; and
 *     cols  = frame                         if gap_extend > 0
 *           = min(frame, la + 1)            otherwise       (the banded calls: min(frame, la + lb + 1))
 *     frame = 1 024; 4 096 where la >= 1 024 in the calls that fill whole matrices (seqalign_fill_batch*, seqalign_nw_batch*,
 *             seqalign_sw_batch*, the legacy one-pair calls)
 * A call is refused before it launches anything, with a message that names these numbers, unless
 *     bound + cols * |gap_extend| <= INT32_MAX.
 * Every scoring with numbers below 2^20 and gaps that cost passes on pairs of up to 1 000 letters; the narrow and the wide banded calls decide
 * alike.  Inside the bound every result is the reference's, bit for bit, up to cell values of 2^31 - 1. */
const char *seqalign_strerror(int code);
/* Text of the last HIP failure on the calling thread ("" if none). */
const char *seqalign_last_error(void);

/* ---- device context --------------------------------------------------------- */
typedef struct seqalign_ctx seqalign_ctx_t;

/* Number of visible gfx950 devices (0 when there is no GPU / no runtime). */
int seqalign_device_count(void);

/* One context per device (one per process in the multi-GPU layout: the batch is
 * sharded by pair index, no collective -- SURVEY 8e). */
int seqalign_ctx_create(int device, seqalign_ctx_t **out);
void seqalign_ctx_destroy(seqalign_ctx_t *ctx);
int seqalign_ctx_device(const seqalign_ctx_t *ctx);

/* ---- scoring, flattened for the device ------------------------------------- */
/* scoring_lookup (src/alignment_scoring.c:133-182) is a pure function of
 * (scoring, a, b); it is flattened ONCE per scoring into a 256-entry
 * char -> (folded char, class) map plus a dense class x class int32 table and
 * uploaded.  The handle stays valid until released or the context dies. */
typedef struct seqalign_dev_scoring seqalign_dev_scoring_t;

int seqalign_scoring_upload(seqalign_ctx_t *ctx, const scoring_t *scoring,
                            int is_sw, seqalign_dev_scoring_t **out);
void seqalign_scoring_release(seqalign_ctx_t *ctx, seqalign_dev_scoring_t *h);

/* ---- batch descriptors -------------------------------------------------------- */
/* Host-side batch: one byte arena + per-pair offsets/lengths (raw chars, not
 * NUL-dependent, exactly what aligner_align takes per pair). */
typedef struct {
  uint64_t n_pairs;
  const char *arena;       /* all sequence bytes                               */
  uint64_t arena_bytes;
  const uint64_t *off_a;   /* [n_pairs] byte offset of seq_a in arena          */
  const uint32_t *len_a;   /* [n_pairs]                                        */
  const uint64_t *off_b;
  const uint32_t *len_b;
} seqalign_batch_t;

/* Device-resident batch + outputs: every pointer is a DEVICE pointer. */
typedef struct {
  uint64_t n_pairs;
  const uint8_t *arena;
  const uint64_t *off_a;
  const uint32_t *len_a;
  const uint64_t *off_b;
  const uint32_t *len_b;
  const uint64_t *mat_off; /* [n_pairs] first cell of pair p in each arena      */
  int32_t *match_scores;   /* three arenas, same per-pair offsets               */
  int32_t *gap_a_scores;
  int32_t *gap_b_scores;
  uint64_t *status;        /* [n_pairs] ~0 = ok, else row-major index of the
                              first cell whose character pair has no score     */
  uint32_t max_len_a;      /* max over the batch (selects columns-per-lane)     */
  uint32_t max_len_b;
} seqalign_dev_batch_t;

/* Which fill kernel family to launch. */
enum {
  SEQALIGN_KERNEL_AUTO = 0,
  SEQALIGN_KERNEL_WAVEFRONT = 1, /* anti-diagonal wavefront, one wave per pair
                                    (north_star's literal schedule); 4-5x slower
                                    than the row sweeps: each lane stores to a
                                    different row.  Kept as an independently
                                    scheduled cross-check; never picked by AUTO.
                                    (Until round 3 every gap_extend > 0 call was
                                    routed here; the row sweeps now take the
                                    trend of their gap_b scan from the right end
                                    for a positive extension, sa_rowsweep.hpp) */
  SEQALIGN_KERNEL_ROWSCAN = 2,   /* row sweep + max-plus prefix scan for gap_b,
                                    rows stored straight from registers        */
  SEQALIGN_KERNEL_STREAM = 3,    /* same sweep, output through an LDS ring as
                                    aligned 1 KiB blocks (len_a <= 1023 and the
                                    three arenas congruent mod 4 KiB; otherwise
                                    the call falls back: AUTO -> STRIPS,
                                    STREAM -> ROWSCAN)                         */
  SEQALIGN_KERNEL_STRIPS = 4,    /* long rows: the 512-column strips of a pair run
                                    as a pipeline of waves, 64 rows apart      */
  SEQALIGN_KERNEL_WGSTREAM = 5   /* rows of 1024..4095 columns: one workgroup per
                                    pair, row split over four waves, shared LDS
                                    ring (fast-path scorings; else ROWSCAN)    */
};

/* THE HOT PATH.  Replaces alignment_fill_matrices (src/alignment.c:28-168) for a
 * whole batch: enqueues the fill on `stream` (a hipStream_t passed as void*,
 * NULL = the context's own stream) and returns without synchronising.
 * WHERE the three output arenas lie decides how fast it runs (it is bound by HBM writes): with arenas from
 * seqalign_arenas_alloc (placed by a measured walk) BASELINE configs[1] runs at 0.82-0.86 of the 8 TB/s peak;
 * with three buffers of the caller's own (hipMalloc, a torch tensor) at 0.65 -- or 0.83 when the allocator happens to hand out
 * memory of different classes: both were seen for the same call on one box (bench.py: roofline.frac_unplaced; round 6:
 * 0.824 / 0.650 / 0.835 in three consecutive processes).  De-phasing the three streams inside the kernel changes nothing
 * (profiles/r06/r06_dephase.txt): it is which memory, not which offsets.  Callers who own the buffers should get them from
 * seqalign_arenas_alloc. */
int seqalign_fill_batch_device(seqalign_ctx_t *ctx,
                               const seqalign_dev_scoring_t *scoring,
                               const seqalign_dev_batch_t *batch, int kernel,
                               void *stream);

/* SW local maxima (replaces the scan of src/smith_waterman.c:152-156 on the
 * device): per pair, the best match_scores cell in reference hit order (score
 * desc, column asc, index asc) and every cell with score >= min_score compacted
 * into cand[cand_off[p] .. +cand_cap[p]) (unsorted; cand_count[p] may exceed the
 * capacity, in which case only the first cand_cap[p] were stored).
 * All pointers are DEVICE pointers. */
typedef struct {
  uint64_t n_pairs;
  const uint32_t *len_a, *len_b;
  const uint64_t *mat_off;
  const int32_t *match_scores;
  int32_t min_score;
  int32_t *best_score;      /* [n_pairs]                                        */
  uint64_t *best_index;     /* [n_pairs] row-major cell index                   */
  uint32_t *cand_count;     /* [n_pairs]                                        */
  const uint64_t *cand_off; /* [n_pairs]                                        */
  const uint32_t *cand_cap; /* [n_pairs]                                        */
  uint32_t *cand_index;     /* compacted cell indices                           */
  int32_t *cand_score;      /* and their scores                                 */
} seqalign_sw_reduce_t;

int seqalign_sw_reduce_device(seqalign_ctx_t *ctx, const seqalign_sw_reduce_t *r,
                              void *stream);

/* Traceback on the device: consumes the matrices a fill left in HBM
 * and applies alignment.c:244-350 per pair, one lane per pair.
 *   NW (seqalign_nw_traceback_device): needleman_wunsch.c:53-132 from the
 *       bottom-right cell to the border.
 *   SW (seqalign_sw_traceback_device): the local alignment ending at
 *       start_index[p] (a match_scores cell, normally best_index from
 *       seqalign_sw_reduce_device), walked until the score is 0 -- what the first
 *       smith_waterman_fetch returns (smith_waterman.c:165-258); out_pos gets
 *       pos_a, pos_b, len_a, len_b (4 per pair).
 * Pair p's two strings are written RIGHT-ALIGNED into
 * out_a/out_b[str_off[p] .. str_off[p]+len_a+len_b): they start at
 * str_off[p]+out_head[p] and are out_len[p] long (no NUL).  status[p] is 0 or a
 * SEQALIGN_E_* code.  All pointers are DEVICE pointers. */
typedef struct {
  const uint64_t *str_off;
  char *out_a, *out_b;
  uint32_t *out_head, *out_len;
  int32_t *out_score;
  uint32_t *status;
  const uint64_t *start_index; /* SW only */
  uint32_t *out_pos;           /* SW only */
} seqalign_trace_t;

int seqalign_nw_traceback_device(seqalign_ctx_t *ctx,
                                 const seqalign_dev_scoring_t *scoring,
                                 const seqalign_dev_batch_t *batch,
                                 const seqalign_trace_t *trace, void *stream);
int seqalign_sw_traceback_device(seqalign_ctx_t *ctx,
                                 const seqalign_dev_scoring_t *scoring,
                                 const seqalign_dev_batch_t *batch,
                                 const seqalign_trace_t *trace, void *stream);

/* ---- host-level convenience (H2D -> fill -> D2H) ---------------------------- */
/* Fills every pair of a HOST batch and copies the matrices back into the three
 * host arenas (cell offsets mat_off[p], host pointer).  Streams the batch in
 * chunks that fit the context's device buffers.  status may be NULL. */
int seqalign_fill_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch,
                        const scoring_t *scoring, int is_sw,
                        const uint64_t *mat_off, int32_t *match_scores,
                        int32_t *gap_a_scores, int32_t *gap_b_scores,
                        uint64_t *status);

/* Global NW over a host batch: GPU fill + traceback (the reference's consumer,
 * src/needleman_wunsch.c:53-145, fresh code).  By default the traceback also runs
 * on the device and only the strings cross PCIe; the option traceback=host copies
 * the matrices back and walks them on the host (north_star's literal split --
 * identical results, PCIe-bound).  For plain scorings (no free / forbidden gaps, no
 * sentinel scores, gap_open <= 0, gap_extend <= 0) and rows up to 1 024 columns (round 5; over 768: from 384 pairs) the
 * device path does not write the matrices at all: the fill leaves one byte of
 * directions per cell -- the answers to alignment_reverse_move's equality tests,
 * src/alignment.c:311-327, taken while the operands are in registers -- and the
 * walk follows them (option nw_dirs=0: three matrices everywhere).
 * Large chunks run as a pipeline of sub-batches (upload / kernels / download on
 * three streams; option subbatches).  Results:
 * score[p], and the two alignment strings of pair p written NUL-terminated at
 * out_a + str_off[p], out_b + str_off[p] (capacity len_a+len_b+1 each). */
int seqalign_nw_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch,
                      const scoring_t *scoring, const uint64_t *str_off,
                      char *out_a, char *out_b, uint32_t *out_len,
                      int32_t *out_score);

/* Local SW over a host batch (src/smith_waterman.c:165-277 semantics, fresh
 * visited mask per pair).  Emits, per pair, successive hits with
 * score >= min_score[p], at most max_hits per pair, into the caller's hit array
 * (hit_cap entries total).
 *   max_hits == 1: GPU fill + GPU reduction + GPU traceback of the best hit.
 *   max_hits >= 2: GPU fill that also reports where the cells >= min_score are (count,
 *       bounding box, columns per row) -> one reverse sweep over each pair's matrices:
 *       a cell is marked by the lowest-ranked walk (reference order: score desc, column
 *       asc, index asc) that arrives at it, so the winners -- and with them every hit of
 *       the pair, in order -- follow from one pass over the rows, bottom to top, without
 *       the sequential procedure of smith_waterman.c:165-277 being run
 *       -> one GPU traceback per wanted hit.  Any max_hits; only the strings cross PCIe.
 *       Plain scorings, rows up to 1 024 columns (513 and up: batches of >= 128 pairs, 769 and up: >= 640; keys
 *       of <= 62 bits): the fill writes match_scores + one byte of directions per cell
 *       instead of the three matrices, the sweep and the walks read those (option
 *       sweep_dirs=0: three matrices everywhere).
 *   option traceback=host: the matrices and the compacted candidates of every
 *       pair are copied back and the hits are enumerated on the host (threaded
 *       over pairs). */
typedef struct {
  uint64_t pair;
  int32_t score;
  uint32_t pos_a, pos_b, len_a, len_b; /* smith_waterman.c:249-255 */
  uint32_t length;                     /* alignment columns */
  uint64_t str_off;                    /* into out_a / out_b */
} seqalign_sw_hit_t;

/* Errors and what has been delivered when they are returned:
 *   SEQALIGN_E_NOMEM   hit_cap or str_cap is too small: the hits that FIT have been delivered first -- a prefix of the
 *                      result in pair order, *n_hits counts them -- then the call stops and reports it;
 *   a pair's own error (SEQALIGN_E_UNKNOWN_PAIR: a character pair without a score, SEQALIGN_E_TRACEBACK): the lowest failing
 *                      pair's code is returned, it takes precedence over E_NOMEM within its chunk, and nothing of that chunk
 *                      is delivered (earlier chunks' hits stay, *n_hits says how many).
 * The packed best-hit path (max_hits == 1, direction bytes) has no separate fill status to fetch: a direction fill is only
 * admitted for scorings in which every character pair has a score, and each walk carries its pair's status home in its own
 * word (sa_batch_sw.hip). */
int seqalign_sw_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch,
                      const scoring_t *scoring, const int32_t *min_score,
                      uint32_t max_hits, seqalign_sw_hit_t *hits,
                      uint64_t hit_cap, uint64_t *n_hits, char *out_a,
                      char *out_b, uint64_t str_cap);

/* ---- asynchronous host-level calls ----------------------------------------------- */
/* A host-level call on one batch is a serial chain (pack, upload, fill, walk, results home, expansion into the caller's strings)
 * of which the kernels are about half; ACROSS batches the chain overlaps: batch k + 1's packing and upload need nothing of batch
 * k's walk and expansion.  The reference has one pair in flight (src/alignment_cmdline.c:611-622); a caller streaming batches
 * submits them and waits for them in order:
 *     seqalign_nw_batch_submit(ctx, &batch[k], sc, ..., &job[k]);   ...   rc = seqalign_job_wait(job[k - 2]);
 * Up to `async_lanes` (option, 1..8, default 3) submitted calls of a context are in flight at once, each on a lane with streams,
 * pinned staging and device scratch of its own (so `async_lanes` times a synchronous call's scratch memory); jobs START in
 * submission order and may finish in any.  A job IS the synchronous call -- same arguments, same results bit for bit -- run with a
 * snapshot of the context's options taken at submit.  Everything passed (the batch's arrays, the scoring, the output buffers) is
 * borrowed until seqalign_job_wait returns.  Submitting is thread-safe; any thread may wait for any job, once.
 *   seqalign_job_wait   blocks until the job has run; returns its SEQALIGN_* code (its text: seqalign_last_error in the waiting
 *                       thread; what it launched: seqalign_ctx_last_call_info of the context) and frees the ticket;
 *   seqalign_job_done   1 when the job has finished (wait will not block), else 0; does not free.
 * seqalign_ctx_destroy runs every submitted job to its end first; tickets never waited for are leaked, not dangling. */
typedef struct seqalign_job seqalign_job_t;
int seqalign_nw_batch_submit(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score,
                             seqalign_job_t **job);
int seqalign_sw_batch_submit(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const int32_t *min_score, uint32_t max_hits, seqalign_sw_hit_t *hits, uint64_t hit_cap,
                             uint64_t *n_hits, char *out_a, char *out_b, uint64_t str_cap, seqalign_job_t **job);
int seqalign_job_wait(seqalign_job_t *job);
int seqalign_job_done(seqalign_job_t *job);

/* ---- several GPUs from one process -------------------------------------------- */
/* The same three calls over n_ctx contexts (normally one per GPU of the node): the
 * pairs are split into n_ctx contiguous index ranges of (nearly) equal DP cells --
 * sum of (len_a+1)*(len_b+1), so ragged batches stay balanced -- context g works on range g
 * from its own host thread, nothing is exchanged between devices (the
 * path shards by pair, no collective).  Results are exactly those of the
 * single-context call.  hits/strings of the SW call come back in pair order; each
 * range gets a share of hit_cap / str_cap proportional to its pairs
 * (SEQALIGN_E_NOMEM if a range overflows its share). */
int seqalign_fill_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx,
                              const seqalign_batch_t *batch, const scoring_t *scoring,
                              int is_sw, const uint64_t *mat_off, int32_t *match_scores,
                              int32_t *gap_a_scores, int32_t *gap_b_scores, uint64_t *status);
int seqalign_nw_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx,
                            const seqalign_batch_t *batch, const scoring_t *scoring,
                            const uint64_t *str_off, char *out_a, char *out_b,
                            uint32_t *out_len, int32_t *out_score);
int seqalign_sw_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx,
                            const seqalign_batch_t *batch, const scoring_t *scoring,
                            const int32_t *min_score, uint32_t max_hits,
                            seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits,
                            char *out_a, char *out_b, uint64_t str_cap);

/* ---- arena placement ----------------------------------------------------------- */
/* Three device buffers of bytes_each for seqalign_dev_batch_t's match_scores /
 * gap_a_scores / gap_b_scores (the reference's three malloc'd matrices,
 * src/alignment.c:183-190, for a whole batch), PLACED in HBM: on MI355X the fill's
 * write pattern (thousands of concurrent sequential streams into three arenas) runs
 * ~25 % slower when all three arenas lie in one "class" of physical memory than when
 * one of them lies in another; three hipMallocs in a row usually
 * land in one class.  Any 4 KiB-aligned device memory is accepted by the fill -- this
 * is only the fast way to get it.  The context's own scratch (host-level entry
 * points) is allocated the same way.
 * How: the arenas are built with the virtual-memory API (hipMemCreate / hipMemMap)
 * from uniform 512 MiB physical chunks.  M and A take the first chunks; further
 * chunks are created (not mapped, not touched: ~10 us each) and every 4 GiB a window
 * of them is mapped as a candidate third arena and timed with the fill's own store
 * pattern against one linear stream; if no candidate reaches the target a second walk
 * moves the SECOND arena the same way (three arenas in three classes are the best there
 * is: the headline kernel at the speed of a memset) (ratio ~0.75: the three disturb each other,
 * 0.98-1.02: one arena in another class, 1.04-1.05: the best there is; the probe repeats to
 * +-2 %).  The first candidate at or above the option arena_quality (default 1.045) ends the walk, otherwise the best one is kept; all other chunks go
 * straight back.  Bounded by the option arena_scan_gib (default 160; 0 = three plain
 * hipMallocs, what the command-line tools use) and by 60 % of the free device
 * memory (re-checked while the walk goes on; a context's own scratch: 25 %, and 16 GiB after its first walk; walks are
 * serialised per device, process-wide); typically 10-60 GiB are held for ~0.1 s.  Arenas under 256 MiB are
 * allocated plainly.  *quality, if not NULL, receives the probe ratio of the result
 * (< 0: not probed); seqalign_arenas_info tells how it was found.  Arenas are meant
 * to be kept and reused.  Free with seqalign_arenas_free (NOT hipFree). */
int seqalign_arenas_alloc(seqalign_ctx_t *ctx, uint64_t bytes_each, void *arenas[3], float *quality);
int seqalign_arenas_free(seqalign_ctx_t *ctx, void *arenas[3]);

#define SEQALIGN_ARENA_MAX_TRIES 96
typedef struct {
  float quality;        /* probe ratio of the arenas handed out (< 0: not probed)          */
  float target;         /* the ratio that would have ended the walk (option arena_quality)  */
  int32_t vmm;          /* 1: built from hipMemCreate chunks, 0: three hipMallocs            */
  uint32_t chunk_mib;   /* chunk size                                                        */
  float depth_gib;      /* how far behind the second arena, in allocation order, the third   */
  float scanned_gib;    /* device memory held at the end of the walks (transient)            */
  float depth_a_gib;    /* where the second walk moved the SECOND arena to (< 0: it stayed    */
                        /* right behind the first)                                           */
  uint32_t tries;       /* candidates timed, both walks                                      */
  uint32_t second_walk_from; /* try_*[second_walk_from ..] belong to the second walk         */
  float try_quality[SEQALIGN_ARENA_MAX_TRIES];    /* their ratios, in order                  */
  float try_depth_gib[SEQALIGN_ARENA_MAX_TRIES];
  float kept_gib;       /* what the process's chunk pool of this device holds after the walk  */
  float seconds;        /* wall clock of seqalign_arenas_alloc: chunk creation, mappings, every timed candidate, releases */
} seqalign_arena_info_t;
/* How the arenas returned by seqalign_arenas_alloc were placed (arenas[0] identifies them). */
int seqalign_arenas_info(seqalign_ctx_t *ctx, void *const arenas[3], seqalign_arena_info_t *info);

/* The chunk pool.  A placement walk creates up to arena_scan_gib of 512 MiB chunks and uses three arenas' worth; the driver
 * clears released VRAM before it hands it out again, so a process whose walk had just given back 160 GiB waited seconds at
 * its next large allocation (round 4: the first seqalign_nw_batch of BASELINE configs[4]'s share 3.7 s).  Up to
 * arena_keep_gib (option, default 16) of the unused chunks therefore stay with the process, per device, and the contexts'
 * large scratch buffers (direction bytes, staging, unplaced arena sets) are mapped from them; chunks of freed buffers and
 * arenas return to the pool.  The pool is emptied when the device's last context is destroyed.
 * seqalign_pool_trim releases everything beyond keep_bytes now (and lowers the cap to it; the next walk raises it again);
 * keep_bytes = UINT64_MAX only queries.  *held_bytes, if not NULL, receives what the pool holds afterwards. */
int seqalign_pool_trim(seqalign_ctx_t *ctx, uint64_t keep_bytes, uint64_t *held_bytes);

/* ---- context options ----------------------------------------------------------- */
/* Everything that steers a context's choices is an option of THAT context.  The defaults are read once, in
 * seqalign_ctx_create, from the environment (SEQALIGN_<KEY>, upper case); afterwards only this call changes
 * them -- nothing below seqalign_ctx_create reads the environment.  Keys and values:
 *   kernel          auto | wavefront | rowscan | stream | strips | wgstream   what SEQALIGN_KERNEL_AUTO means
 *   traceback       device | host           where seqalign_nw_batch / seqalign_sw_batch walk the matrices
 *   trace_kernel    auto | lane | wave      the device walker
 *   sweep_mode      auto | pair | strips    multi-hit SW: one wave per pair / per strip
 *   sweep_strip     0 | 64 | 128 | 256      columns per strip       sweep_cpl  0 | 1 | 2 | 4
 *   chunk_bytes     0 | >= 1 MiB            device memory one host-level chunk may use
 *   async_lanes     0 (= 3) | 1 .. 8        submitted calls in flight per context (seqalign_*_batch_submit)
 *   walk_group      0 | 1 | 4 | 8           walks per wave of the device walker on LDS tiles (4 / 8: in lockstep, vector state); 0: four on
 *                                           direction bytes laid out in blocks (NW, best hit; rows <= 512 columns), else one wave per walk
 *   dirs_local      1 | 0                   seqalign_nw_batch / seqalign_sw_batch(max_hits = 1) on direction bytes: the byte holds the cell's own comparisons and the
 *                                           walker resolves the state it arrives in (cheaper to write; 0: the older form everywhere)
 *   walk_tile       0 | 32 | 64             that walker's tile edge in bytes (0: 32 for global walks -- fewer lines per reload --, 64 for best-hit walks)
 *   walk_stage      1 | 0                   that walker sends a wave's moves home as one run of whole lines out of LDS (0: two pieces per walk)
 *   subbatches      0 (by size) .. 256      sub-batches a chunk of seqalign_nw_batch is pipelined in (1 = off)
 *   nw_dirs, sweep_dirs  1 | 0              direction bytes instead of the three matrices where they apply (above)
 *   pack16          1 | 0 | 2               direction-byte fills take two pairs per wave in packed int16 where scores fit int16 --
 *                                           pairs of EQUAL shape share a wave: a chunk of one shape, or a ragged chunk whose pairs
 *                                           are paired up by shape on the host (the others: one per wave in the same launch, NW;
 *                                           a wave to themselves, SW): for chunks of > 1 024 pairs (ragged: >= 2 048) | never | whatever the size
 *   quad            0 | 1 | 2               the NW and the SW best-hit fill with FOUR pairs per wave (32 lanes a couple of pairs; chunks of
 *                                           one shape, rows up to 192 columns): for chunks of >= 4 096 (NW) / 16 384 (SW) pairs | never |
 *                                           whatever the size
 *   walk_overlap    0 | 1                   seqalign_nw_batch (direction bytes): walks on their own stream beside the next fills (round 4:
 *                                           off -- beside the four-pairs-per-wave fills the walks cost more than they hide)
 *   nw_moves        1 | 0                   the walks on direction bytes send home two bits per alignment column (which string has
 *                                           a gap there) and the host expands them against the caller's sequences, instead of the
 *                                           gapped strings (seqalign_nw_batch; seqalign_sw_batch: also ONE launch + wait for all
 *                                           hits of a chunk, the walks launched before the counts are seen); DESIGN.md 3.5d, 3.6c
 *   zero_copy       auto | 0..3             that path's kernels read the packed sequences (1) / write the moves (2) in pinned host
 *                                           memory in place; auto: moves in place when the walks run one wave each
 *   sweep_ev        1 | 0                   the direction-byte sweep carries a walk as one word key << 2 | state
 *   arena_scan_gib  0 .. 1024               arena_quality  0.5 .. 1.5    (seqalign_arenas_alloc)
 *   arena_keep_gib  0 .. 1024               (the chunk pool, seqalign_pool_trim)
 *   arena_free_pct  10 .. 90                share of the memory free at its start that a walk of seqalign_arenas_alloc may hold (60)
 *   upload_slices   0 .. 16                 seqalign_nw_batch: slices a sub-batch's sequences are packed and uploaded in (0 = 1: measured,
 *                                           more slices cost what they overlap)
 *   long_block_rows 0 | N >= 1              seqalign_*_align_long: rows per block and between checkpoint rows (0: sized from the chunk budget)
 *   band_strip_cols 0 | 64 | 128 | 256 | 512   seqalign_*_banded_wide: columns per strip of the band's pipeline of waves (0: 512 from 512 pairs
 *                                           on, else 256, see "wide banded calls")
 *   cpl, wpb, lds_pad, reduce_depth, sweep_trace, timing   tuning experiments / development aids
 * Numbers are integers and nothing else ("abc", "1x", "" are refused, not read as 0); switches take 1 / 0, true / false, on / off,
 * yes / no.  Returns SEQALIGN_E_ARG for an unknown key or a value outside the key's range (nothing changes then). */
int seqalign_ctx_set_option(seqalign_ctx_t *ctx, const char *key, const char *value);

/* The value in force (as text: what seqalign_ctx_set_option would take) -- for callers that change an option for a
 * while and put it back.  Returns SEQALIGN_E_ARG for an unknown key or when cap is too small. */
int seqalign_ctx_get_option(const seqalign_ctx_t *ctx, const char *key, char *value, size_t cap);

/* ---- what the last call launched ------------------------------------------------ */
/* Which kernels the context's last call (any entry point above that launches) put on the device, and for how many
 * pairs / walks each: the fills of src/alignment.c:28-168 come in several forms (three matrices, direction bytes, two
 * pairs per wave in packed int16 ...) chosen per chunk from the scoring and the shapes, and results are identical
 * whichever runs -- so a test (or a user wondering where the time goes) asks HERE which one did.  launches[k] /
 * items[k] are indexed by SEQALIGN_K_*; a call that chunks or pipelines its batch adds up all its launches. */
enum {
  SEQALIGN_K_FILL_WAVEFRONT = 0,   /* three matrices, sa_fill_wavefront.hip                                        */
  SEQALIGN_K_FILL_ROWSCAN,         /* ... sa_fill_rowscan.hip                                                      */
  SEQALIGN_K_FILL_STREAM,          /* ... sa_fill_stream.hip (the headline kernel)                                 */
  SEQALIGN_K_FILL_STRIPS,          /* ... sa_fill_strips.hip                                                       */
  SEQALIGN_K_FILL_WGSTREAM,        /* ... sa_fill_wgstream.hip                                                     */
  SEQALIGN_K_FILL_NW_DIRS,         /* NW, direction bytes only, one pair per wave (items: pairs)                   */
  SEQALIGN_K_FILL_NW_DIRS_X2,      /* NW, direction bytes only, two pairs per wave in packed int16                 */
  SEQALIGN_K_FILL_SW_DIRS,         /* SW, match_scores + direction bytes, one pair per wave                        */
  SEQALIGN_K_FILL_SW_DIRS_X2,      /* SW, match_scores + direction bytes, two pairs per wave                       */
  SEQALIGN_K_FILL_SW_BEST_X2,      /* SW best hit: direction bytes + the best cell, two pairs per wave             */
  SEQALIGN_K_SW_REDUCE,            /* sa_reduce.hip: the separate max-reduction over match_scores                  */
  SEQALIGN_K_SW_BOX,               /* sa_reduce.hip: candidates' box / rows from match_scores in HBM               */
  SEQALIGN_K_SWEEP_REGS,           /* multi-hit sweep on three matrices, rows in registers                         */
  SEQALIGN_K_SWEEP_LDS,            /* ... winners of two rows in LDS (wide pairs)                                  */
  SEQALIGN_K_SWEEP_STRIPS,         /* ... one wave per strip (few wide pairs)                                      */
  SEQALIGN_K_SWEEP_DIRS,           /* multi-hit sweep on match_scores + direction bytes, one pair per wave         */
  SEQALIGN_K_SWEEP_DIRS_X2,        /* (reserved: two pairs per wave measured slower, never launched)               */
  SEQALIGN_K_WALK_LANE,            /* traceback on three matrices, one lane per walk (items: walks)                */
  SEQALIGN_K_WALK_WAVE,            /* ... one wave per walk, LDS tiles                                             */
  SEQALIGN_K_WALK_DIRS_LANE,       /* traceback on direction bytes, strings out, one lane per walk                 */
  SEQALIGN_K_WALK_DIRS_TILE,       /* ... one wave per walk, LDS tiles                                             */
  SEQALIGN_K_WALK_MOVES_LANE,      /* traceback on direction bytes, two bits per column out (host/sa_moves.c)      */
  SEQALIGN_K_WALK_MOVES_TILE,      /* ... one wave per walk                                                        */
  SEQALIGN_K_FILL_NW_DIRS_X4,      /* NW, direction bytes only, FOUR pairs per wave (32 lanes a couple of pairs)   */
  SEQALIGN_K_FILL_SW_BEST_X4,      /* SW best hit: direction bytes + the best cell, four pairs per wave            */
  SEQALIGN_K_SCORE_ROWS,           /* score only (seqalign_*_score_batch), one pair per wave, rows <= 1 024 columns */
  SEQALIGN_K_SCORE_STRIPS,         /* ... wider rows: strips of 512 columns, one wave each (items: pairs)          */
  SEQALIGN_K_SCORE_CROSS,          /* score only over two sets (seqalign_*_score_cross), one wave per (query, target) */
  SEQALIGN_K_SCORE_SELECT,         /* top-k search (seqalign_*_score_search): a tile's best targets per query (items: rows) */
  SEQALIGN_K_LONG_FORWARD,         /* pairs of any size (seqalign_*_align_long): score strips + checkpoint rows     */
  SEQALIGN_K_LONG_BLOCK,           /* ... the three matrices of one block, from its checkpoint (one launch per block) */
  SEQALIGN_K_LONG_WALK,            /* ... the traceback over one block                                              */
  SEQALIGN_K_COUNT
};
#define SEQALIGN_K_MAX 32
#if defined(__cplusplus)
static_assert(SEQALIGN_K_COUNT <= SEQALIGN_K_MAX, "seqalign_call_info_t has SEQALIGN_K_MAX slots");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(SEQALIGN_K_COUNT <= SEQALIGN_K_MAX, "seqalign_call_info_t has SEQALIGN_K_MAX slots");
#endif
typedef struct {
  uint32_t launches[SEQALIGN_K_MAX];
  uint64_t items[SEQALIGN_K_MAX];
} seqalign_call_info_t;
int seqalign_ctx_last_call_info(const seqalign_ctx_t *ctx, seqalign_call_info_t *out);
/* "fill_stream", "fill_nw_dirs_x2", ... ; NULL for a kind that does not exist */
const char *seqalign_kernel_kind_name(int kind);
/* The table above is full (SEQALIGN_K_COUNT == SEQALIGN_K_MAX) and seqalign_call_info_t is ABI, so kernels added since
 * are counted in a second record of the same shape, indexed by SEQALIGN_KX_*.  The outermost entry point of a call clears
 * both records; a call that launches none of the kernels below leaves this one all zero. */
enum {
  /* (the banded SW calls are counted under these three as well: see "banded SW"; so are the wide banded calls, whose
   * band_score / band_fill items are the (pair, strip) waves that swept at least one row: see "wide banded calls") */
  SEQALIGN_KX_BAND_SCORE = 0,      /* banded NW, score only (seqalign_nw_score_banded), one pair per wave (items: pairs) */
  SEQALIGN_KX_BAND_FILL,           /* banded NW, M / A / B of every band cell (seqalign_nw_align_banded)                  */
  SEQALIGN_KX_BAND_WALK,           /* ... the traceback over a chunk's bands, one lane per pair                           */
  SEQALIGN_KX_COUNT
};
#define SEQALIGN_KX_MAX 32
typedef struct {
  uint32_t launches[SEQALIGN_KX_MAX];
  uint64_t items[SEQALIGN_KX_MAX];
} seqalign_call_info_ext_t;
int seqalign_ctx_last_call_info_ext(const seqalign_ctx_t *ctx, seqalign_call_info_ext_t *out);
/* "band_score", "band_fill", "band_walk"; NULL for a kind that does not exist */
const char *seqalign_kernel_kind_ext_name(int kind);

/* ---- CIGAR -------------------------------------------------------------------- */
/* The reference has no CIGAR output (its result is the pair of gapped strings, src/alignment.h:33-40); this
 * is the derived format: run-length encoding of the alignment's columns with seq_a as the query and seq_b as
 * the reference -- both letters: M (extended = 0) or '=' / 'X' (extended != 0; letters compared as they are,
 * or case-folded when case_insensitive), '-' in result_b: I (insertion to the reference), '-' in result_a: D.
 * Writes a NUL-terminated string; returns its length, or (size_t)-1 when cap is too small or a column has a
 * gap in both strings.  Host only, no device involved. */
size_t seqalign_cigar(const char *result_a, const char *result_b, size_t length, int extended,
                      int case_insensitive, char *out, size_t cap);

/* The batch calls with CIGAR as their output (north_star: "identical CIGAR/alignment strings").  Same alignments, same order, same
 * query convention as seqalign_cigar above -- seq_a is the QUERY, seq_b the REFERENCE: a column with '-' in result_b is I, with '-'
 * in result_a is D.  format: SEQALIGN_CIGAR_M (M / I / D) or SEQALIGN_CIGAR_EQX (= / X / I / D; letters compared case-folded unless
 * scoring->case_sensitive).  On plain scorings the device walks come home as two bits per alignment column and the
 * host run-length encodes those bits: the gapped strings are never written, and a read's "150M" is 5 bytes where its strings are 302.
 *   seqalign_nw_batch_cigar: pair p's CIGAR NUL-terminated at cigar + cigar_off[p], capacity cigar_off[p + 1] - cigar_off[p] (cigar_off
 *     has n_pairs + 1 entries; SEQALIGN_E_NOMEM when a pair's does not fit: no CIGAR is longer than 2 (len_a + len_b) + 1 bytes),
 *     cigar_len[p] = its strlen, out_score[p] as seqalign_nw_batch.  A global alignment's CIGAR covers both sequences completely
 *     (leading / trailing gaps are I / D runs, as the reference's strings have them, src/needleman_wunsch.c:117-132).
 *   seqalign_sw_batch_cigar: as seqalign_sw_batch; hit h's CIGAR NUL-terminated at cigar + hits[h].str_off, hits back to back;
 *     hits[h].length stays the number of alignment columns, pos_a / pos_b / len_a / len_b say where the hit lies. */
#define SEQALIGN_CIGAR_M 1
#define SEQALIGN_CIGAR_EQX 2
int seqalign_nw_batch_cigar(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int format,
                            const uint64_t *cigar_off, char *cigar, uint32_t *cigar_len, int32_t *out_score);
int seqalign_sw_batch_cigar(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                            const int32_t *min_score, uint32_t max_hits, int format, seqalign_sw_hit_t *hits,
                            uint64_t hit_cap, uint64_t *n_hits, char *cigar, uint64_t cigar_cap);
int seqalign_nw_batch_cigar_submit(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int format,
                                   const uint64_t *cigar_off, char *cigar, uint32_t *cigar_len, int32_t *out_score,
                                   seqalign_job_t **job);   /* (asynchronous: seqalign_job_wait, above) */
/* ... and over several contexts (GPUs), as seqalign_nw_batch_multi / seqalign_sw_batch_multi */
int seqalign_nw_batch_cigar_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  int format, const uint64_t *cigar_off, char *cigar, uint32_t *cigar_len, int32_t *out_score);
int seqalign_sw_batch_cigar_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const int32_t *min_score, uint32_t max_hits, int format, seqalign_sw_hit_t *hits,
                                  uint64_t hit_cap, uint64_t *n_hits, char *cigar, uint64_t cigar_cap);

/* ---- score only ------------------------------------------------------------------ */
/* Optimal score per pair, no alignment.  NW: the global score (what seqalign_nw_batch's out_score holds).
 * SW: the best cell in reference hit order -- score, and the 1-based matrix coordinates of that cell
 * (end_a = i, end_b = j: the best local alignment ends with seq_a[i-1], seq_b[j-1]); score 0 and (0,0)
 * when no cell scores above 0.  No limit on len_a * len_b.
 * Nothing per cell is written to device memory: rows of up to 1 024 columns are swept by one wave per pair, wider rows by
 * strips of 512 columns that hand their last column to the next strip (8 bytes per row and strip).  Batches are chunked
 * by sequence bytes; 4 (NW) or 12 (SW) bytes per pair come back.  Same argument checks and scoring admission
 * (SEQALIGN_E_DOMAIN) as seqalign_nw_batch / seqalign_sw_batch, without their 2^31-cell cap.  A character pair without a
 * score (SEQALIGN_E_UNKNOWN_PAIR): the lowest failing pair's code is returned and named in seqalign_last_error. */
int seqalign_nw_score_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                            int32_t *out_score);
int seqalign_sw_score_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                            int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b);
/* ... over several contexts (GPUs): contiguous ranges of nearly equal cells, results exactly the single-context call's */
int seqalign_nw_score_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                  const scoring_t *scoring, int32_t *out_score);
int seqalign_sw_score_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch,
                                  const scoring_t *scoring, int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b);
/* ---- SW hit spans: where the best local hit starts and ends, no traceback ------------ */
/* Per pair the fields of the first hit of seqalign_sw_batch(min_score = 1, max_hits = 1) without its strings: score; pos_a,
 * pos_b (0-based: the cell in which the reference's walk from the best cell reaches score 0 -- its tie order GAP_A, GAP_B,
 * MATCH, not merely some optimal start); len_a, len_b, so that pos + len is seqalign_sw_score_batch's end_a / end_b.  All
 * five are 0 when no cell scores above 0.  No limit on len_a * len_b: the lengths accepted are seqalign_sw_score_batch's.
 * One forward pass carries the spans beside the scores; nothing per cell is written to device memory.  Rows of up to 512
 * columns are swept by one wave per pair, wider rows by strips of 512 columns.  Device bytes per pair: len_a + len_b + 72,
 * and for rows over 512 columns 32 x (strips - 1) x (len_b + 1) of hand-off plus 36 per strip, strips = ceil(len_a / 512);
 * batches are chunked by these bytes, 20 bytes per pair and the error word come back.
 * Argument checks, scoring admission (SEQALIGN_E_DOMAIN) and SEQALIGN_E_UNKNOWN_PAIR (the lowest failing pair's code is
 * returned and named in seqalign_last_error) are seqalign_sw_score_batch's.  SEQALIGN_E_TRACEBACK cannot occur: in SW a
 * positive cell always has a predecessor the walker accepts.  The launches are recorded as "score_rows" /
 * "score_strips" (items: pairs).
 * Over two sets: seqalign_sw_span_cross (the span matrices) and seqalign_sw_span_search (top k with spans) below.
 * Not in this call: no _submit or command-line form, and no option steers it (banded, up to 512 diagonals:
 * seqalign_sw_span_banded below). */
int seqalign_sw_span_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int32_t *out_score,
                           uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b);
/* ... over several contexts (GPUs): contiguous ranges of nearly equal cells, results exactly the single-context call's */
int seqalign_sw_span_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                 int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a,
                                 uint32_t *out_len_b);
/* Kernel time of seqalign_sw_span_batch (seq-align_amd/tools/sw_span_bench.py), the sibling of seqalign_score_time_ms: the
 * batch (one chunk) is uploaded once, then its kernels run `repeats` times, each launch between two HIP events. */
int seqalign_sw_span_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                             float *ms_each);
/* ---- NW alignment statistics: identity counts of the global alignment, no traceback ---- */
/* For every pair, over the alignment seqalign_nw_batch returns for it (the reference's end pick at the corner cell and
 * alignment_reverse_move's tie order GAP_A, GAP_B, MATCH -- not merely some optimal alignment):
 *   out_score[p]       what seqalign_nw_score_batch returns;
 *   out_matches[p]     the columns that hold a letter of both sequences whose two letters are equal after the scoring's own case
 *                      folding (scoring_t.case_sensitive); wildcards and substitution scores play no part;
 *   out_mismatches[p]  the other columns that hold a letter of both.
 * From these: aligned columns = matches + mismatches; alignment length = len_a + len_b - matches - mismatches; gap columns =
 * len_a + len_b - 2 (matches + mismatches); identity = matches / alignment length, or over the shorter sequence, as the
 * caller prefers.  A pair with len_a == 0 or len_b == 0 has both counts 0.
 *   Nothing is stored per cell and nothing is walked: the two counters travel forward beside the three values of a cell
 * (DESIGN.md 3.21).  Device memory per pair: the sequences, 64 bytes of descriptors, status and results, and for rows over 512
 * columns 32 bytes per row and strip of 512 columns of hand-off; 12 bytes per pair come home.  No 2^31-cell cap.
 *   Lengths, argument checks, scoring admission (SEQALIGN_E_DOMAIN) and SEQALIGN_E_UNKNOWN_PAIR are
 * seqalign_nw_score_batch's.  SEQALIGN_E_TRACEBACK ("pair P: traceback failed") is returned for the lowest pair whose end
 * state has no walk, in the order in which seqalign_nw_batch reports the two errors (the lowest failing pair's code; on one
 * pair the missing score first).  Over whole matrices every pair keeps the alignment that puts all of seq_a and then all of
 * seq_b against gaps, whatever no_mismatches / no_gaps_in_a / no_gaps_in_b forbid, so within the admitted domain no pair
 * takes that path.  On an error the outputs are unspecified beyond the chunks already delivered.
 *   Not here: a search form, a wide banded form, _cross_multi, _submit, the command-line tools, gap-open counts.  The banded
 * form is seqalign_nw_stats_banded below.  SW statistics: seqalign_sw_stats_batch below. */
int seqalign_nw_stats_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int32_t *out_score,
                            uint32_t *out_matches, uint32_t *out_mismatches);
/* ... over several contexts (GPUs): contiguous ranges of nearly equal cells, results exactly the single-context call's */
int seqalign_nw_stats_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches);
/* Kernel time of seqalign_nw_stats_batch (seq-align_amd/tools/nw_stats_bench.py), the sibling of seqalign_sw_span_time_ms */
int seqalign_nw_stats_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                              float *ms_each);
/* ---- SW alignment statistics: hit span and identity counts of the best local hit in one pass, no traceback ---- */
/* For every pair, over the first hit of seqalign_sw_batch(min_score = 1, max_hits = 1) -- the best cell in hit order and the
 * walk of alignment_reverse_move from it, tie order GAP_A, GAP_B, MATCH, not merely some optimal hit:
 *   out_score, out_pos_a, out_pos_b, out_len_a, out_len_b   exactly seqalign_sw_span_batch's five;
 *   out_matches[p]     the columns of that hit's strings that hold a letter of both sequences whose two letters are equal
 *                      after the scoring's own case folding (scoring_t.case_sensitive); substitution scores, wildcards and
 *                      no_mismatches play no part in which bucket a column falls into;
 *   out_mismatches[p]  the other columns that hold a letter of both.
 * All seven are 0 when no cell scores above 0.  From these, BLAST-style: aligned columns = matches + mismatches; alignment
 * length = len_a + len_b - matches - mismatches (the hit's len_a, len_b); gap columns = len_a + len_b - 2 (matches +
 * mismatches); identity = matches / alignment length; qstart = pos_a + 1, qend = pos_a + len_a, sstart = pos_b + 1, send =
 * pos_b + len_b.
 *   One forward pass, nothing stored per cell and nothing walked: beside the three values of a cell travel two words, the
 * cell in which the walk stops as x | y << 16 and matches | mismatches << 16.  So both sequences of every
 * pair must have at most SEQALIGN_SW_STATS_MAX_LEN letters: a longer one is SEQALIGN_E_TOO_LARGE with the lowest such pair
 * named in seqalign_last_error, found from the descriptors with the other argument checks, before the context is touched and
 * before any device work.  There is no cap on len_a * len_b: 65 535 x 65 535 is legal.
 *   Device bytes per pair: len_a + len_b + 80, and for rows over 512 columns 32 x (strips - 1) x (len_b + 1) of hand-off plus
 * 36 per strip, strips = ceil(len_a / 512) -- seqalign_sw_span_batch's plus 8 bytes of results; batches are chunked by these
 * bytes, 28 bytes per pair and the error word come back.  Argument checks, scoring admission (SEQALIGN_E_DOMAIN) and
 * SEQALIGN_E_UNKNOWN_PAIR are seqalign_sw_span_batch's; SEQALIGN_E_TRACEBACK cannot occur.  The launches are recorded as
 * "score_rows" / "score_strips" (items: pairs).
 *   Not here: a search form, _cross_multi, _submit, the command-line tools.  Gap-open counts: seqalign_sw_gaps_batch below.
 * Sequences over 65 535 letters:
 * seqalign_sw_counts_batch below returns score, end and the two counts at any length, seqalign_sw_span_batch start and length
 * (a four-word payload does not fit: DESIGN.md 3.22, 3.32).  The banded form is seqalign_sw_stats_banded below. */
#define SEQALIGN_SW_STATS_MAX_LEN 65535u
int seqalign_sw_stats_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int32_t *out_score,
                            uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b,
                            uint32_t *out_matches, uint32_t *out_mismatches);
/* ... over several contexts (GPUs): contiguous ranges of nearly equal cells, results exactly the single-context call's; the
 * length limit names the pair's index in the whole batch */
int seqalign_sw_stats_batch_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a,
                                  uint32_t *out_len_b, uint32_t *out_matches, uint32_t *out_mismatches);
/* Kernel time of seqalign_sw_stats_batch (seq-align_amd/tools/sw_stats_bench.py), the sibling of seqalign_sw_span_time_ms */
int seqalign_sw_stats_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                              float *ms_each);
/* ---- SW identity counts at any length: score, end and identity counts of the best local hit, no traceback ---- */
/* seqalign_sw_stats_batch without its length limit and without the start of the hit.  For every pair, over the first hit of
 * seqalign_sw_batch(min_score = 1, max_hits = 1):
 *   out_score, out_end_a, out_end_b   byte for byte seqalign_sw_score_batch's three: the best match_scores cell in hit order,
 *                      1-based; 0, 0, 0 when no cell is above 0;
 *   out_matches[p], out_mismatches[p]   the two counts of seqalign_sw_stats_batch: the letter columns of that hit's strings,
 *                      split by whether the two letters are equal after the scoring's own case folding; substitution scores,
 *                      wildcards and no_mismatches play no part; both 0 where there is no hit.
 * For every batch seqalign_sw_stats_batch accepts, the counts equal its sixth and seventh outputs and end_a / end_b its
 * pos + len.  There is NO limit on the sequence lengths: the two payload words of the sweep are the two counts, a full 32-bit
 * word each, and a walk has at most min(len_a, len_b) letter columns, so neither can wrap.  The counts do not
 * depend on where the walk stops, so seqalign_sw_span_batch on the same batch supplies pos and len for any pair.  The recipe:
 * up to 65 535 letters one seqalign_sw_stats_batch sweep gives all seven integers; past that, two sweeps -- this call and
 * seqalign_sw_span_batch.
 *   Argument checks and their order, scoring admission (SEQALIGN_E_DOMAIN), SEQALIGN_E_UNKNOWN_PAIR and the chunk rules are
 * seqalign_sw_span_batch's; SEQALIGN_E_TRACEBACK cannot occur.  Device bytes per pair are the span call's: len_a + len_b + 72,
 * and for rows over 512 columns 32 x (strips - 1) x (len_b + 1) of hand-off plus 36 per strip, strips = ceil(len_a / 512);
 * batches are chunked by these bytes (option chunk_bytes), 20 bytes per pair and the error word come back.  The launches are
 * recorded as "score_rows" / "score_strips" (items: pairs); the call adds no kernel kind.
 *   Not here: cross, search, _multi, _submit and command-line forms; one call that returns all seven integers at any length;
 * gap-open counts (seqalign_sw_gaps_batch below).  Banded: seqalign_sw_counts_banded and seqalign_sw_counts_banded_wide below. */
int seqalign_sw_counts_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int32_t *out_score,
                             uint32_t *out_end_a, uint32_t *out_end_b, uint32_t *out_matches, uint32_t *out_mismatches);
/* Kernel time of seqalign_sw_counts_batch (seq-align_amd/tools/sw_counts_bench.py), as seqalign_sw_stats_time_ms */
int seqalign_sw_counts_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                               float *ms_each);
/* ---- SW gap-run counts at any length: score, end and the gap opens of the best local hit, no traceback ---- */
/* The gapopen field of a BLAST-style tabular line without the strings.  For every pair, over the first hit of
 * seqalign_sw_batch(min_score = 1, max_hits = 1):
 *   out_score, out_end_a, out_end_b   byte for byte seqalign_sw_score_batch's three: the best match_scores cell in hit order,
 *                      1-based; 0, 0, 0 when no cell is above 0;
 *   out_gap_runs_a[p]  the number of maximal runs of '-' in that hit's string a;
 *   out_gap_runs_b[p]  the same in its string b; both 0 where there is no hit.  BLAST's gapopen is their sum.  An insertion
 *                      directly against a deletion is two runs, one in each string.  The number of gap COLUMNS follows from
 *                      seqalign_sw_span_batch's lengths and seqalign_sw_counts_batch's counts
 *                      (len_a + len_b - 2 (matches + mismatches)), so no word is spent on it.
 * A run is counted at its first column, not at an "open" move of the scoring: with gap_extend > 0 a gap can extend out of a
 * cell whose score is 0, where the hit begins, and that run counts as every other.  There is NO limit on the
 * sequence lengths: both counts are full 32-bit words and a hit has fewer than len_a + len_b < 2^31 columns.  The recipe for a
 * full tabular line (pident, length, mismatch, gapopen, qstart, qend, sstart, send, score): up to 65 535 letters
 * seqalign_sw_stats_batch and this call; past that seqalign_sw_span_batch, seqalign_sw_counts_batch and this call.
 *   Argument checks and their order, scoring admission (SEQALIGN_E_DOMAIN), SEQALIGN_E_UNKNOWN_PAIR, the chunk rules, the
 * device bytes per pair and the 20 bytes per pair that come back are seqalign_sw_counts_batch's (the span call's) exactly;
 * SEQALIGN_E_TRACEBACK cannot occur.  The launches are recorded as "score_rows" / "score_strips" (items: pairs); the call adds
 * no kernel kind.
 *   Not here: NW gap runs; cross, search, _multi, _submit and command-line forms; one call that returns a whole tabular line.
 * Banded: seqalign_sw_gaps_banded and seqalign_sw_gaps_banded_wide below. */
int seqalign_sw_gaps_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int32_t *out_score,
                           uint32_t *out_end_a, uint32_t *out_end_b, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b);
/* Kernel time of seqalign_sw_gaps_batch (seq-align_amd/tools/sw_gaps_bench.py), as seqalign_sw_counts_time_ms */
int seqalign_sw_gaps_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                             float *ms_each);
/* ---- banded SW hit spans: start and end of the best local hit inside a band, no traceback ---- */
/* seqalign_sw_span_batch over the banded SW matrices: the five integers a mapper reports per read at the cost of a banded
 * sweep, nothing stored per cell and no walk.
 *   Band and matrices are seqalign_sw_score_banded's ("banded SW" below), word for word: the caller's bounds diag_lo[p] <=
 *   diag_hi[p], anywhere in int32, clipped to [-len_b, len_a]; every cell outside the band and every border cell holds 0 in
 *   all three matrices; a band that is empty after clipping is legal and gives five zeros.
 *   Per pair the fields of the hit seqalign_sw_align_banded(min_score = 1) delivers, without its strings: score; pos_a, pos_b
 *   (0-based: the cell in which alignment_reverse_move's walk from the best band cell reaches score 0, tie order GAP_A,
 *   GAP_B, MATCH); len_a, len_b, so that pos + len is seqalign_sw_score_banded's end_a / end_b.  All five are 0 when no band
 *   cell is above 0.  With gap_extend > 0 the start may lie one diagonal OUTSIDE the band, exactly as the align call's does:
 *   the walk steps onto a cell that reads 0 and stops there.
 *   SEQALIGN_E_ARG, SEQALIGN_E_DOMAIN, SEQALIGN_E_NO_DEVICE, SEQALIGN_E_NOMEM   as seqalign_sw_score_banded
 *   SEQALIGN_E_UNKNOWN_PAIR   a character pair without a score INSIDE the band only (lowest failing pair named)
 *   SEQALIGN_E_TOO_LARGE      a pair whose clipped width exceeds SEQALIGN_SPAN_BAND_MAX_WIDTH (pair and width named), or
 *                             len_a + len_b >= 2^31; found from lengths and bounds alone, before any device work
 *   SEQALIGN_E_TRACEBACK      cannot occur: a positive band cell always has a predecessor the walker accepts, a cell outside
 *                             the band being one that holds 0 and stops the walk
 * No 2^31-cell cap.  Device bytes per pair: len_a + len_b + 88 (the score call's and the wider result record); chunks are cut
 * within the option chunk_bytes; 20 bytes per pair and the error word come home.  One wave per pair, 1 .. 6 or 8 band
 * diagonals per lane.  seqalign_ctx_last_call_info_ext: the call adds no kind, its launches are counted under band_score, one
 * per width class of a chunk.
 * Not in this call: widths over 512 -- the two-word span sweep does not fit one wave's registers at 12 and 16 columns per lane
 * (DESIGN.md 3.18); seqalign_sw_span_banded_wide ("wide banded calls" below) takes any width -- and no cross, search (the
 * unbanded call has both: seqalign_sw_span_cross, seqalign_sw_span_search), _multi,
 * _submit or command-line form, and no option steers it. */
#define SEQALIGN_SPAN_BAND_MAX_WIDTH 512
int seqalign_sw_span_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                            const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score,
                            uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b);
/* Timing hook (tools/sw_span_banded_bench.py), the sibling of seqalign_sw_band_score_time_ms for seqalign_sw_span_banded:
 * one chunk, `repeats` launches between HIP events */
int seqalign_sw_span_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each);
/* ---- banded SW statistics: hit span and identity counts of the best local hit inside a band, no traceback ---- */
/* seqalign_sw_stats_batch over the banded SW matrices: the seven integers of a BLAST-style tabular line per read at the cost
 * of a banded sweep, nothing stored per cell and no walk.
 *   Band and matrices are seqalign_sw_score_banded's ("banded SW" below), word for word: bounds anywhere in int32, clipped to
 *   [-len_b, len_a]; every cell outside the band and every border cell holds 0 in all three matrices.
 *   Per pair the fields of the hit seqalign_sw_align_banded(min_score = 1) delivers, and the counts of THAT hit's strings:
 *   out_score, out_pos_a, out_pos_b, out_len_a, out_len_b   exactly seqalign_sw_span_banded's five;
 *   out_matches, out_mismatches   counted as seqalign_sw_stats_batch counts them: the columns of the hit's strings that hold
 *                      a letter of both sequences, split by whether the two letters are equal after the scoring's own case
 *                      folding; substitution scores, wildcards and no_mismatches play no part.
 *   All seven are 0 when no band cell is above 0, or when the band is empty after clipping.  With gap_extend > 0 the start may
 *   lie one diagonal OUTSIDE the band, as seqalign_sw_span_banded's does: a cell outside the band is a stop that has counted
 *   nothing.
 * Refused before any device work, with a context that is never dereferenced, in this order:
 *   1. SEQALIGN_E_ARG        a NULL argument (the timing hook: or repeats <= 0);
 *   2. seqalign_sw_span_banded's checks of batch and band: SEQALIGN_E_ARG for an unreadable batch or diag_lo[p] > diag_hi[p]
 *      (pair named); SEQALIGN_E_TOO_LARGE for a clipped width over SEQALIGN_SPAN_BAND_MAX_WIDTH (pair and width named) or
 *      len_a + len_b >= 2^31 -- the lowest such pair;
 *   3. SEQALIGN_E_TOO_LARGE  a sequence of more than SEQALIGN_SW_STATS_MAX_LEN letters, seqalign_sw_stats_batch's message
 *      ("pair P: seq_a has N letters, SW statistics take at most 65535") -- the lowest such pair.
 *   So a batch that is too wide in one pair and too long in another reports the width, whichever pair comes first.
 * SEQALIGN_E_DOMAIN, SEQALIGN_E_UNKNOWN_PAIR (a character pair without a score INSIDE the band only) and the chunk rules are
 * seqalign_sw_span_banded's; SEQALIGN_E_TRACEBACK cannot occur.  Device bytes per pair: len_a + len_b + 96 (the span call's 88
 * and two result words); 28 bytes per pair and the error word come home.  One wave per pair, 1 .. 6 or 8 band diagonals per
 * lane.  seqalign_ctx_last_call_info_ext: the call adds no kind, its launches are counted under band_score,
 * one per width class of a chunk.
 * Widths over 512: seqalign_sw_stats_banded_wide ("wide banded calls" below).
 * Not in this call (banded NW statistics: seqalign_nw_stats_banded and seqalign_nw_stats_banded_wide below): cross, search,
 * _multi, _submit, the command-line tools; gap-open counts are seqalign_sw_gaps_banded's. */
int seqalign_sw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score,
                             uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b,
                             uint32_t *out_matches, uint32_t *out_mismatches);
/* Timing hook (tools/sw_stats_banded_bench.py), the sibling of seqalign_sw_span_band_time_ms for seqalign_sw_stats_banded:
 * one chunk, `repeats` launches between HIP events; a batch that does not fit one chunk is SEQALIGN_E_ARG */
int seqalign_sw_stats_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                   const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each);
/* ---- banded SW identity counts at any length: score, end and identity counts of the best hit inside a band ---- */
/* seqalign_sw_counts_batch over the banded SW matrices: percent identity of a long read against its window at the cost of a
 * banded sweep, nothing stored per cell and no walk.
 *   Band and matrices are seqalign_sw_score_banded's ("banded SW" below), word for word.
 *   out_score, out_end_a, out_end_b   byte for byte seqalign_sw_score_banded's three;
 *   out_matches, out_mismatches       the two counts of seqalign_sw_stats_banded: the letter columns of the strings of the hit
 *                      seqalign_sw_align_banded(min_score = 1) delivers, split by whether the two letters are equal after the
 *                      scoring's own case folding.
 *   All five are 0 when no band cell is above 0, or when the band is empty after clipping.  For every batch
 *   seqalign_sw_stats_banded accepts the counts equal its sixth and seventh outputs and the ends its pos + len.
 * NO limit on the sequence lengths (two full count words); seqalign_sw_span_banded on the same arguments
 * supplies pos and len for any pair.
 * Band geometry, clipping, argument checks, their order and every error are seqalign_sw_span_banded's, with a context that is
 * never dereferenced before them: SEQALIGN_E_ARG (a NULL argument, an unreadable batch, diag_lo[p] > diag_hi[p]);
 * SEQALIGN_E_TOO_LARGE (a clipped width over SEQALIGN_SPAN_BAND_MAX_WIDTH = 512, or len_a + len_b >= 2^31; the lowest such
 * pair); SEQALIGN_E_DOMAIN by the same bound; SEQALIGN_E_UNKNOWN_PAIR for a character pair without a score INSIDE the band
 * only; SEQALIGN_E_NOMEM with the bytes named.  Device bytes per pair: len_a + len_b + 88 (the span call's); 20 bytes per
 * pair and the error word come home.  One wave per pair, 1 .. 6 or 8 band diagonals per lane.  The launches are counted
 * under band_score, one per width class of a chunk.  Widths over 512: seqalign_sw_counts_banded_wide below.
 * Not here: cross, search, _multi, _submit, the command-line tools; gap-open counts are seqalign_sw_gaps_banded's. */
int seqalign_sw_counts_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                              const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                              uint32_t *out_end_b, uint32_t *out_matches, uint32_t *out_mismatches);
/* Timing hook (tools/sw_counts_bench.py), as seqalign_sw_stats_band_time_ms for seqalign_sw_counts_banded */
int seqalign_sw_counts_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                    const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each);
/* ---- banded SW gap-run counts at any length: score, end and the gap opens of the best hit inside a band ---- */
/* seqalign_sw_gaps_batch over the banded SW matrices: the gapopen field of a long read against its window at the cost of a
 * banded sweep, nothing stored per cell and no walk.
 *   Band and matrices are seqalign_sw_score_banded's ("banded SW" below), word for word.
 *   out_score, out_end_a, out_end_b   byte for byte seqalign_sw_score_banded's three;
 *   out_gap_runs_a, out_gap_runs_b    the numbers of maximal runs of '-' in strings a and b of the hit
 *                      seqalign_sw_align_banded(min_score = 1) delivers.  A cell outside the band ends the hit as a cell of
 *                      score 0 does: a gap that extends out of it begins its run inside the band.
 *   All five are 0 when no band cell is above 0, or when the band is empty after clipping.
 * NO limit on the sequence lengths (two full words).
 * Band geometry, clipping, argument checks, their order, every error, the device bytes per pair (len_a + len_b + 88) and the
 * 20 bytes per pair that come home are seqalign_sw_counts_banded's (the span call's) exactly, the cap of
 * SEQALIGN_SPAN_BAND_MAX_WIDTH = 512 clipped diagonals included.  One wave per pair, 1 .. 6 or 8 band diagonals per lane.  The
 * launches are counted under band_score, one per width class of a chunk.  Widths over 512: seqalign_sw_gaps_banded_wide below.
 * Not here: NW gap runs, cross, search, _multi, _submit, the command-line tools. */
int seqalign_sw_gaps_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                            const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                            uint32_t *out_end_b, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b);
/* Timing hook (tools/sw_gaps_bench.py), as seqalign_sw_counts_band_time_ms for seqalign_sw_gaps_banded */
int seqalign_sw_gaps_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each);
/* ---- banded NW statistics: identity counts of the global alignment inside a band, no traceback ---- */
/* seqalign_nw_stats_batch over the banded NW matrices: score, matches and mismatches of long similar pairs at the cost of a
 * banded sweep, nothing stored per cell and no walk.
 *   band[p] = w is seqalign_nw_score_banded's argument with the same geometry ("banded NW" below):
 *       d_lo = max(-len_b, min(0, len_a - len_b) - w)      d_hi = min(len_a, max(0, len_a - len_b) + w)
 *   and the matrices are its matrices: every cell outside the band holds the NW floor in all three.
 *   out_score[p]   seqalign_nw_score_banded's value exactly.
 *   A pair that has an alignment inside its band gets the one seqalign_nw_align_banded returns: out_matches[p] /
 *   out_mismatches[p] are the counts over THAT alignment's strings, split as seqalign_nw_stats_batch splits them (letters
 *   compared after the scoring's own case folding; substitution scores and wildcards play no part).  So when the unbanded
 *   alignment stays inside the band all three are seqalign_nw_stats_batch's.
 *   A pair that has no alignment inside its band: SEQALIGN_E_TRACEBACK ("pair P: traceback failed (no alignment inside the
 *   band)"), the lowest such pair named, ordered with SEQALIGN_E_UNKNOWN_PAIR as seqalign_nw_stats_batch orders the two (the
 *   lowest failing pair's code).
 *   This is decided as seqalign_nw_stats_batch decides it, by the sticky mark the sweep carries beside the counts: the end
 *   pick's state, or a state the walk from it would pass through, has every candidate below the NW floor (or none: a blocked
 *   letter pair, a cell outside the band).  It is NOT decided by the end value: with a scoring of large numbers a real score
 *   lies below INT32_MIN / 2, far above the floor, and such a pair has its alignment and gets its counts.
 *   It differs from what seqalign_nw_align_banded does on one family of pairs: under no_mismatches the align call's walker
 *   reads a blocked letter pair as score 0, floor + 0 == floor lets it step from a cell at the floor to any other, cells
 *   outside the band included, and the walk can "succeed" with an end value at the floor.  Such strings are no alignment of
 *   the banded problem (they hold a blocked letter pair or leave the band); this call returns SEQALIGN_E_TRACEBACK for those
 *   pairs.  The reverse does not occur: no pair this call refuses has a walk that stays inside the band.
 * Refused before any device work, with a context that is never dereferenced, in seqalign_nw_score_banded's order:
 *   1. SEQALIGN_E_ARG        a NULL argument (the timing hook: or repeats <= 0);
 *   2. SEQALIGN_E_ARG        an unreadable batch;
 *   3. SEQALIGN_E_TOO_LARGE  len_a + len_b >= 2^31, or a width over SEQALIGN_SPAN_BAND_MAX_WIDTH = 512 diagonals ("pair P: a
 *                            band of N diagonals, at most 512 are supported") -- the lowest such pair.
 * No limit on the sequence lengths (the two counts are full words; SEQALIGN_SW_STATS_MAX_LEN plays no part) and no cell cap.
 * SEQALIGN_E_DOMAIN and SEQALIGN_E_UNKNOWN_PAIR (a character pair without a score INSIDE the band only) are
 * seqalign_nw_score_banded's.  Device bytes per pair: len_a + len_b + 72 (descriptors, status and three result words); chunks
 * are cut within the option chunk_bytes; 12 bytes per pair and the error word come home.  One wave per pair, 1 .. 6 or 8 band
 * diagonals per lane.  seqalign_ctx_last_call_info_ext: the call adds no kind, its launches are counted
 * under band_score, one per width class of a chunk.
 * Widths over 512: seqalign_nw_stats_banded_wide ("wide banded calls" below).
 * Not in this call: cross, search, _multi, _submit, the command-line tools, gap-open counts. */
int seqalign_nw_stats_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const uint32_t *band, int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches);
/* Timing hook (tools/nw_stats_banded_bench.py), the sibling of seqalign_band_score_time_ms for seqalign_nw_stats_banded:
 * one chunk, `repeats` launches between HIP events; a batch that does not fit one chunk is SEQALIGN_E_ARG */
int seqalign_nw_stats_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                   const uint32_t *band, int repeats, float *ms_each);
/* ---- long pairs: alignments past the 2^31-cell cap --------------------------------- */
/* The alignments of seqalign_nw_batch and of seqalign_sw_batch with max_hits = 1 -- same arguments, capacities and results,
 * byte for byte: score, both gapped strings and, SW, the hit's pos_a / pos_b / len_a / len_b / length -- for pairs of any
 * size (len_a + len_b < 2^32 - 1, else SEQALIGN_E_TOO_LARGE).  The three matrices are never held whole: a forward pass (the
 * score-only strips) stores M, A and B at every R-th row (12 B x (len_a + 1) per checkpoint row) and finds the SW best
 * cell; then, block by block from the end cell, rows [checkpoint below the walk, the walk's row] x columns [0, the walk's
 * column] are recomputed from their checkpoint and walked (alignment_reverse_move's decision order).  Device memory per pair:
 *   12 (len_a + 1) (floor((len_b - 1) / R) + min(R, len_b) + 1) + 8 (ceil(len_a / 512) - 1) (len_b + 1) + 3 (len_a + len_b)
 * bytes; R (rows per block, fewer than 2^31 cells) is the option long_block_rows, or (0, the default) the largest that fits
 * the context's chunk budget (option chunk_bytes).  A pair that does not fit even so: SEQALIGN_E_NOMEM, seqalign_last_error
 * gives the bytes needed.  Pairs run one after another, small ones included (this is for few large pairs; batches of many
 * small pairs belong to seqalign_nw_batch / seqalign_sw_batch).  Argument checks (SEQALIGN_E_ARG, SEQALIGN_E_TOO_LARGE)
 * come before any device work; scoring admission (SEQALIGN_E_DOMAIN) and a character pair without a score
 * (SEQALIGN_E_UNKNOWN_PAIR, the lowest failing pair named in seqalign_last_error) are the score calls'.  SW: hit_cap or
 * str_cap too small -- the hits that fit are delivered, *n_hits counts them, SEQALIGN_E_NOMEM.
 * seqalign_ctx_last_call_info: kinds long_forward, long_block (one launch per block), long_walk. */
int seqalign_nw_align_long(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                           const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len, int32_t *out_score);
int seqalign_sw_align_long(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                           const int32_t *min_score, seqalign_sw_hit_t *hits, uint64_t hit_cap, uint64_t *n_hits,
                           char *out_a, char *out_b, uint64_t str_cap);
/* ---- banded NW: score and alignment inside a diagonal band ------------------------- */
/* Global alignment restricted to a band of diagonals, for long similar sequences.  band[p] = w (any w >= 0) gives pair p,
 * with la = len_a, lb = len_b, the band
 *     d_lo = max(-lb, min(0, la - lb) - w)      d_hi = min(la, max(0, la - lb) + w)
 *     cell (i, j) (column i of seq_a, row j of seq_b) is in the band  iff  d_lo <= i - j <= d_hi;  width = d_hi - d_lo + 1
 * so (0, 0) and (la, lb) are in every band and a band that covers the whole matrix has width la + lb + 1.  The banded
 * matrices are the reference's recurrence (src/alignment.c:28-168, borders included) in which every cell outside the band
 * holds the NW floor in all three matrices; the banded alignment is needleman_wunsch.c's end pick and
 * alignment_reverse_move over those matrices.  Nothing is rounded to a kernel's frame, nothing is adaptive.  When the
 * unbanded alignment of a pair stays inside its band, score and strings are seqalign_nw_batch's byte for byte; otherwise
 * the score is <= the unbanded one.  A scoring that forbids moves (no_mismatches, no_gaps_in_*) may leave NO alignment
 * inside a band: seqalign_nw_align_banded then returns SEQALIGN_E_TRACEBACK (lowest failing pair named in
 * seqalign_last_error); seqalign_nw_score_banded returns the end cell's value as it is, below INT32_MIN / 2 then.  The value
 * alone does not tell: with a scoring of large numbers a real score can lie below INT32_MIN / 2 as well.
 * Results, capacities and str_off exactly as seqalign_nw_score_batch / seqalign_nw_batch.  No 2^31-cell cap.
 *   SEQALIGN_E_ARG          NULL arguments, unreadable batch
 *   SEQALIGN_E_TOO_LARGE    a pair whose width exceeds SEQALIGN_BAND_MAX_WIDTH (found from lengths and bands alone, before
 *                           any device work; pair named), or len_a + len_b >= 2^31
 *   SEQALIGN_E_DOMAIN, SEQALIGN_E_NO_DEVICE   as the long calls
 *   SEQALIGN_E_UNKNOWN_PAIR a character pair without a score INSIDE the band (lowest failing pair named); the same
 *                           characters outside the band raise nothing
 *   SEQALIGN_E_NOMEM        a pair that does not fit the chunk budget alone; seqalign_last_error gives the bytes needed
 * Chunks are cut by device bytes within the option chunk_bytes.  Per pair: the score call len_a + len_b + 64; the align
 * call 12 (len_b + 1) width (M, A, B of the band's cells: row j holds diagonals d_lo .. d_hi, cell (i, j) at
 * j (width - 1) + i - d_lo) + 3 (len_a + len_b) + 96.
 * seqalign_ctx_last_call_info_ext: band_score / band_fill + band_walk. */
#define SEQALIGN_BAND_MAX_WIDTH 1024
int seqalign_nw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const uint32_t *band, int32_t *out_score);
int seqalign_nw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const uint32_t *band, const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len,
                             int32_t *out_score);
/* Timing hook (tools/align_banded_bench.py), the banded sibling of seqalign_score_time_ms: the batch (one chunk) is uploaded
 * once, then the score call's launches run `repeats` times between HIP events; ms_each[r] = kernel time of repeat r. */
int seqalign_band_score_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                const uint32_t *band, int repeats, float *ms_each);
/* ---- banded SW: the best local hit within a range of diagonals per pair -------------- */
/* Local alignment restricted to the diagonals a seed or an index points at.  Pair p gets two signed bounds diag_lo[p] <=
 * diag_hi[p]; cell (i, j) (column i of seq_a, row j of seq_b) is IN THE BAND  iff  diag_lo[p] <= i - j <= diag_hi[p].  The
 * bounds are the caller's and may lie anywhere, wholly left or right of the main diagonal included: the band is NOT anchored
 * to the two corners as the NW band is.  They are clipped to [-len_b, len_a] (d_lo = max(diag_lo, -len_b), d_hi = min(diag_hi,
 * len_a)); width = d_hi - d_lo + 1 is the clipped count of diagonals.  A band that is empty after clipping (d_lo > d_hi) is
 * legal: score 0, no hit.
 *   The banded SW matrices are the reference's recurrence (src/alignment.c:28-168, is_sw = 1) in which every cell outside the
 *   band holds the SW floor, 0, in all three matrices (the SW borders are 0 too: for SW "border" and "outside the band" read the
 *   same).  The banded best hit is smith_waterman.c's first hit over those matrices: the best match_scores cell in hit order
 *   (score descending, column ascending, index ascending), walked by alignment_reverse_move until the score is 0.  Nothing is
 *   rounded to a kernel's frame, nothing is adaptive.
 * What follows: a band that covers every inner cell gives the unbanded matrices; banded values are <= the unbanded ones
 * everywhere; when the unbanded best hit's walk visits band cells only, start and end cell included, the banded hit is the
 * unbanded one field for field and byte for byte, otherwise its score is not above it.  With gap_open + gap_extend <= 0 and
 * gap_extend <= 0 the banded hit's own walk never leaves the band; with a positive gap_extend it can (cells outside read 0).
 *   seqalign_sw_score_banded   seqalign_sw_score_batch's results: score, end_a, end_b of the best band cell, 1-based; 0 and
 *                              (0, 0) when no band cell is above 0
 *   seqalign_sw_align_banded   seqalign_sw_align_long's results and capacities: at most one hit per pair, delivered iff its
 *                              score is > 0 and >= min_score[p], hits in pair order; hit_cap or str_cap too small: the hits
 *                              that fit are delivered, *n_hits counts them, SEQALIGN_E_NOMEM
 *   SEQALIGN_E_ARG          NULL arguments, unreadable batch, a pair with diag_lo > diag_hi as given (pair named)
 *   SEQALIGN_E_TOO_LARGE    a pair whose clipped width exceeds SEQALIGN_BAND_MAX_WIDTH (pair and width named), or len_a +
 *                           len_b >= 2^31; like SEQALIGN_E_ARG found from lengths and bounds alone, before any device work
 *   SEQALIGN_E_DOMAIN, SEQALIGN_E_NO_DEVICE   as the other SW calls
 *   SEQALIGN_E_UNKNOWN_PAIR a character pair without a score INSIDE the band (lowest failing pair named; such a cell keeps 0
 *                           in match_scores); the same characters outside the band raise nothing
 *   SEQALIGN_E_NOMEM        a pair that does not fit the chunk budget alone; seqalign_last_error gives the bytes needed
 * No 2^31-cell cap.  Chunks are cut by device bytes within the option chunk_bytes.  Per pair: the score call len_a + len_b +
 * 80; the align call 12 rows width + 3 (len_a + len_b) + 128, rows = the rows that have inner band cells,
 *     max(0, min(len_b, len_a - d_lo) - max(1, 1 - d_hi) + 1)      (0 when len_a = 0 or the band is empty)
 * (M, A, B of those rows: row j holds diagonals d_lo .. d_hi).  32 bytes per pair and the strings come home.
 * seqalign_ctx_last_call_info_ext: the second launch record's table is pinned, so these calls add no kind -- their launches
 * are counted under band_score / band_fill + band_walk (one band_score or band_fill launch per width class of a chunk), whose
 * names fit; which family a record belongs to is known from the call that was made. */
int seqalign_sw_score_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                             uint32_t *out_end_b);
int seqalign_sw_align_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                             const int32_t *diag_lo, const int32_t *diag_hi, const int32_t *min_score, seqalign_sw_hit_t *hits,
                             uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b, uint64_t str_cap);
/* Timing hook (tools/align_banded_sw_bench.py), the sibling of seqalign_band_score_time_ms for seqalign_sw_score_banded */
int seqalign_sw_band_score_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                   const int32_t *diag_lo, const int32_t *diag_hi, int repeats, float *ms_each);
/* ---- wide banded calls: banded calls at any band width ------------------------------ */
/* The banded calls above hold a pair's whole band in one wave and stop at SEQALIGN_BAND_MAX_WIDTH diagonals.  These four take
 * the argument lists of their siblings unchanged and accept ANY width: a pair's band is cut into strips of columns, one
 * wave per strip, the waves of a pair working as a pipeline that hands a strip's last column on to the strip on its right
 * (so one long pair, too, uses many waves).  The band definitions of "banded NW" and "banded SW" apply word for word -- the
 * clamps, d_lo / d_hi, every cell outside the band at the floor, the end pick, the walk, the results and their capacities --
 * and for every batch the narrow call accepts, the wide call returns the same bytes, the same status and names the same pair
 * in seqalign_last_error.  Only the width rule differs:
 *   SEQALIGN_E_TOO_LARGE    len_a + len_b >= 2^31 only (from lengths alone, before the context is touched)
 *   SEQALIGN_E_ARG          as the siblings: NULL arguments, unreadable batch, (SW) diag_lo > diag_hi with the pair named
 *   SEQALIGN_E_NOMEM        a pair that does not fit the chunk budget alone (the bytes named): the align calls are bounded by
 *                           memory only
 *   SEQALIGN_E_HIP          "band strip hand-off timed out" with the pair named: a wave waited for the strip on its left while
 *                           for over 2 s NO strip of that pair published progress (only a device preempted for that long
 *                           can cause it: some strip of a pair always runs); nothing is delivered
 * Device bytes per pair, chunks cut within the option chunk_bytes: what the sibling call needs (see there: the align calls
 * 12 rows width + ..., the same layout) plus the pipeline's scratch
 *     strips (8 width + 20) + 20,      strips = max(1, ceil(len_a / S)),  S = columns per strip
 * (chunks are also cut so that pairs-rounded-up-to-8 times the chunk's largest strip count stays within 2^28 workgroups; per
 * strip a hand-off column of `width` entries of 8 bytes -- max(M, A) and B of the strip's last column on the rows where
 * that cell is in the band --, a progress word and a best-cell entry; per pair two descriptors and a word that counts its strips'
 * publications).
 * S is the option band_strip_cols; 0, the default, takes 512 for batches of 512 pairs or more and 256 for fewer, what was
 * fastest where it was measured.  Results do not depend on S.
 * seqalign_ctx_last_call_info_ext: band_score, or band_fill + band_walk, one band_score / band_fill launch per chunk; their
 * items count the (pair, strip) waves that swept at least one row -- the strips that hold a column with an inner band cell.
 * No _multi, _submit or timing-hook variants. */
int seqalign_nw_score_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const uint32_t *band, int32_t *out_score);
int seqalign_nw_align_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const uint32_t *band, const uint64_t *str_off, char *out_a, char *out_b, uint32_t *out_len,
                                  int32_t *out_score);
int seqalign_sw_score_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                                  uint32_t *out_end_b);
int seqalign_sw_align_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const int32_t *diag_lo, const int32_t *diag_hi, const int32_t *min_score, seqalign_sw_hit_t *hits,
                                  uint64_t hit_cap, uint64_t *n_hits, char *out_a, char *out_b, uint64_t str_cap);
/* The wide form of seqalign_nw_stats_banded: its argument list and contract word for word -- the band, seqalign_nw_score_banded's
 * score, the counts over the strings seqalign_nw_align_banded(_wide) returns, the case folding, SEQALIGN_E_TRACEBACK by the mark
 * (not the end value) and its order with SEQALIGN_E_UNKNOWN_PAIR, no limit on the lengths -- under the wide calls' width rule above: any width,
 * SEQALIGN_E_TOO_LARGE for len_a + len_b >= 2^31 only, SEQALIGN_E_NOMEM and SEQALIGN_E_HIP as above, and for every batch the
 * narrow call accepts the same bytes, the same status and the same pair named.  The refusals before the context is touched are
 * seqalign_nw_score_banded_wide's, in its order.  A hand-off entry carries the two values, whose the first is and their two
 * payloads, 32 bytes, so the device bytes per pair are
 *     len_a + len_b + 72 + strips (32 width + 20) + 20,      strips = max(1, ceil(len_a / S)).
 * The option band_strip_cols steers S as above; launches are counted under band_score, one per chunk, items = the busy (pair,
 * strip) waves.  Kernel: sa_band_nw_stats_strips.hip.  One pair of 100 000 letters at 511 diagonals runs on
 * many waves here and on one in the narrow call; for many short pairs within 512 diagonals the narrow call is the faster one.
 * The SW form is seqalign_sw_stats_banded_wide below.  No cross, search, _multi, _submit, timing-hook or command-line form. */
int seqalign_nw_stats_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const uint32_t *band, int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches);
/* The wide form of seqalign_sw_stats_banded: its argument list and contract word for word -- the band and its clipping, the
 * banded matrices, the best cell in hit order and the seven integers of its walk, seven zeros where no band cell is above 0 and
 * for an empty band, a start one diagonal outside the band under gap_extend > 0, the case folding, SEQALIGN_E_UNKNOWN_PAIR for a
 * character pair without a score inside the band only -- under the wide calls' width rule above: any clipped width is legal,
 * SEQALIGN_E_NOMEM and SEQALIGN_E_HIP as above, and for every batch the narrow call accepts the same bytes, the same status
 * and the same pair named.  Refused before the context is touched, in this order: a NULL argument (SEQALIGN_E_ARG); per pair,
 * the lowest first, an unreadable batch or diag_lo[p] > diag_hi[p] (SEQALIGN_E_ARG) and len_a + len_b >= 2^31
 * (SEQALIGN_E_TOO_LARGE); then a sequence of more than SEQALIGN_SW_STATS_MAX_LEN letters (SEQALIGN_E_TOO_LARGE, the narrow
 * call's message, the lowest such pair) -- the narrow call's two passes without the width check.  A hand-off entry carries the
 * two values, whose the first is and the two packed words of each, 32 bytes; a strip's best cell travels with its two words,
 * 32 bytes; so the device bytes per pair are
 *     len_a + len_b + 96 + strips (32 width + 36) + 20,      strips = max(1, ceil(len_a / S)).
 * The option band_strip_cols steers S as above; launches are counted under band_score, one per chunk, items = the busy (pair,
 * strip) waves.  Kernel: sa_band_frame.hpp by sa_band_stats.hip.  For many short pairs within 512 diagonals the narrow
 * call is the faster one.  Past 65 535 letters the five span integers come from seqalign_sw_span_banded_wide and the two
 * counts from seqalign_sw_counts_banded_wide, both below; no cross, search, _multi, _submit, timing-hook or command-line
 * form. */
int seqalign_sw_stats_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score,
                                  uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b,
                                  uint32_t *out_matches, uint32_t *out_mismatches);
/* The wide form of seqalign_sw_span_banded: its argument list and contract word for word -- the band and its clipping to
 * [-len_b, len_a], the banded matrices, the best band cell in hit order and the five fields of the hit
 * seqalign_sw_align_banded(_wide)(min_score = 1) delivers, five zeros where no band cell is above 0 and for an empty band, a start
 * one diagonal outside the band under gap_extend > 0, SEQALIGN_E_UNKNOWN_PAIR for a character pair without a score inside the
 * band only -- under the wide calls' width rule above: any clipped width is legal, SEQALIGN_E_NOMEM and SEQALIGN_E_HIP as above,
 * and for every batch the narrow call accepts the same bytes, the same status and the same pair named.  There is NO limit on the
 * lengths: the payload is two full words, the stop cell's x and y.  For every batch seqalign_sw_stats_banded_wide accepts the
 * five equal its first five; score and pos + len equal seqalign_sw_score_banded_wide's three, always.  Refused before the context
 * is touched, in this order: a NULL argument (SEQALIGN_E_ARG); per pair, the lowest first, an unreadable batch or diag_lo[p] >
 * diag_hi[p] (SEQALIGN_E_ARG, the narrow call's message) and len_a + len_b >= 2^31 (SEQALIGN_E_TOO_LARGE).  A hand-off entry
 * carries the two values, whose the first is and the span of each, 32 bytes; a strip's best cell travels with its span, 32
 * bytes; so the device bytes per pair are
 *     len_a + len_b + 88 + strips (32 width + 36) + 20,      strips = max(1, ceil(len_a / S)).
 * The option band_strip_cols steers S as above; launches are counted under band_score, one per chunk, items = the busy (pair,
 * strip) waves.  Kernel: sa_band_frame.hpp by sa_band_span.hip; all four strip widths run without scratch.  This is the
 * cheap way to the start of a hit in long sequences with an indel-widened band: the align call stores 12 bytes per band cell,
 * the wide score call gives the end only.  For many short pairs within 512 diagonals the narrow call is the faster one.
 * No option, kind or constant of its own; no cross, search, _multi, _submit, timing-hook or command-line form. */
int seqalign_sw_span_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                 const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score,
                                 uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b);
/* The wide form of seqalign_sw_counts_banded: its argument list and contract word for word -- score and end byte for byte
 * seqalign_sw_score_banded_wide's, the two counts seqalign_sw_stats_banded_wide's wherever that call accepts the batch, five
 * zeros where no band cell is above 0 and for an empty band -- under the wide calls' width rule above: any clipped width is
 * legal, SEQALIGN_E_NOMEM and SEQALIGN_E_HIP (the hand-off timeout) as above, and for every batch the narrow call accepts the
 * same bytes, the same status and the same pair named.  There is NO limit on the lengths.  Checks, their order and every
 * error are seqalign_sw_span_banded_wide's: a NULL argument (SEQALIGN_E_ARG); per pair, the lowest first, an unreadable batch
 * or diag_lo[p] > diag_hi[p] (SEQALIGN_E_ARG) and len_a + len_b >= 2^31 (SEQALIGN_E_TOO_LARGE).  Hand-off and best entries
 * are the span call's, 32 bytes each, with the two counts where its span is; so the device bytes per pair are the span call's:
 *     len_a + len_b + 88 + strips (32 width + 36) + 20,      strips = max(1, ceil(len_a / S)).
 * The option band_strip_cols steers S as above; launches are counted under band_score, one per chunk, items = the busy (pair,
 * strip) waves.  Kernel: sa_band_frame.hpp by sa_band_counts.hip.  With seqalign_sw_span_banded_wide on the
 * same arguments this gives the seven integers of a tabular line for a 200 kb read in its band: two sweeps, nothing stored per
 * cell.  No cross, search, _multi, _submit, timing-hook or command-line form. */
int seqalign_sw_counts_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                   const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                                   uint32_t *out_end_b, uint32_t *out_matches, uint32_t *out_mismatches);
/* The wide form of seqalign_sw_gaps_banded: its argument list and contract word for word -- score and end byte for byte
 * seqalign_sw_score_banded_wide's, the two run counts those of seqalign_sw_align_banded_wide(min_score = 1)'s strings, five
 * zeros where no band cell is above 0 and for an empty band -- under the wide calls' width rule above: any clipped width is
 * legal, and for every batch the narrow call accepts the same bytes, the same status and the same pair named.  There is NO
 * limit on the lengths.  Checks, their order, every error, hand-off and best entries (32 bytes each, the two run counts where
 * the span is) and the device bytes per pair are seqalign_sw_counts_banded_wide's (the span call's) exactly:
 *     len_a + len_b + 88 + strips (32 width + 36) + 20,      strips = max(1, ceil(len_a / S)).
 * The option band_strip_cols steers S as above; launches are counted under band_score, one per chunk, items = the busy (pair,
 * strip) waves.  Kernel: sa_band_frame.hpp by sa_band_gaps.hip.  With seqalign_sw_span_banded_wide and
 * seqalign_sw_counts_banded_wide on the same arguments this completes the tabular line of a 200 kb read in its band: three
 * sweeps, nothing stored per cell.  No cross, search, _multi, _submit, timing-hook or command-line form. */
int seqalign_sw_gaps_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                 const int32_t *diag_lo, const int32_t *diag_hi, int32_t *out_score, uint32_t *out_end_a,
                                 uint32_t *out_end_b, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b);
/* ---- score matrices: every query against every target, score only ---------------- */
/* A set of sequences: one byte arena, per-sequence offset and length (raw chars, as seqalign_batch_t). */
typedef struct {
  uint64_t n_seqs;
  const char *arena;
  uint64_t arena_bytes;
  const uint64_t *off;   /* [n_seqs] */
  const uint32_t *len;   /* [n_seqs] */
} seqalign_seqset_t;
/* The result of seqalign_*_score_batch on the batch of n_queries * n_targets pairs whose pair p = q * n_targets + t has
 * seq_a = query q and seq_b = target t -- without that batch: the outputs are dense, row-major [n_queries][n_targets]
 * (64-bit indexing), end_a indexes the query and end_b the target.  Each distinct sequence goes to the device once per tile
 * (tiles: query ranges x target ranges within the context's chunk budget); queries of up to 1 024 columns run one wave per
 * (query, target), longer ones the strips of seqalign_*_score_batch.  Argument checks and scoring admission
 * (SEQALIGN_E_DOMAIN) are the score-batch calls'; no cell cap.  n_queries * n_targets overflowing uint64_t:
 * SEQALIGN_E_ARG, before any array is read.  No queries or no targets: SEQALIGN_OK, nothing written.  A character pair
 * without a score: SEQALIGN_E_UNKNOWN_PAIR, and seqalign_last_error names the failing pair with the lowest
 * q * n_targets + t as "query Q, target T: ...".  On an error the outputs are unspecified. */
int seqalign_nw_score_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                            const scoring_t *scoring, int32_t *out_score);
int seqalign_sw_score_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                            const scoring_t *scoring, int32_t *out_score, uint32_t *out_end_a, uint32_t *out_end_b);
/* ... over several contexts (GPUs): contiguous query ranges of nearly equal cells, each context writes its own rows;
 * results exactly the single-context call's */
int seqalign_nw_score_cross_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                  const seqalign_seqset_t *targets, const scoring_t *scoring, int32_t *out_score);
int seqalign_sw_score_cross_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                  const seqalign_seqset_t *targets, const scoring_t *scoring, int32_t *out_score,
                                  uint32_t *out_end_a, uint32_t *out_end_b);
/* ---- top-k score search: the best targets of every query ------------------------------------------------------------ */
#define SEQALIGN_SEARCH_MAX_K 1024
typedef struct {
  uint32_t target;       /* index into the target set */
  int32_t score;
  uint32_t end_a, end_b; /* SW: as seqalign_sw_score_cross (1-based best cell; 0, 0 when score 0); NW: 0, 0 */
} seqalign_search_hit_t;
/* For query q: every target t with score[q][t] >= min_score, where score is what seqalign_*_score_cross returns on the same
 * sets, ordered by score descending, then target ascending; the first min(k, count) go to hits[q * k ...] with the cross
 * call's end_a / end_b, and n_hits[q] is how many were written (slots past it are unspecified).  The order is total: the
 * result does not depend on tiling, chunk_bytes or the number of contexts.  min_score INT32_MIN: no filter.  Only the hit
 * lists leave the device (selection runs there per tile; queries over 1 024 columns are selected on the host).
 * SEQALIGN_E_ARG: NULL arguments, k == 0 or k > SEQALIGN_SEARCH_MAX_K, n_targets > UINT32_MAX, n_queries x n_targets
 * overflowing uint64_t -- all before any array is read.  No targets: SEQALIGN_OK with every n_hits[q] = 0.  No queries:
 * SEQALIGN_OK, nothing written.  A character pair without a score: SEQALIGN_E_UNKNOWN_PAIR, named as the cross call
 * names it. */
int seqalign_nw_score_search(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                             const scoring_t *scoring, uint32_t k, int32_t min_score, seqalign_search_hit_t *hits,
                             uint32_t *n_hits);
int seqalign_sw_score_search(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                             const scoring_t *scoring, uint32_t k, int32_t min_score, seqalign_search_hit_t *hits,
                             uint32_t *n_hits);
/* ... over several contexts: contiguous query ranges cut as seqalign_*_score_cross_multi cuts them; results exactly the
 * single-context call's */
int seqalign_nw_score_search_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                   const seqalign_seqset_t *targets, const scoring_t *scoring, uint32_t k, int32_t min_score,
                                   seqalign_search_hit_t *hits, uint32_t *n_hits);
int seqalign_sw_score_search_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                   const seqalign_seqset_t *targets, const scoring_t *scoring, uint32_t k, int32_t min_score,
                                   seqalign_search_hit_t *hits, uint32_t *n_hits);
/* ---- SW hit spans over two sets: span matrices and a top-k search with spans ----------------------------------------- */
/* seqalign_sw_span_cross: the result of seqalign_sw_span_batch on the batch whose pair q * n_targets + t is (query q, target
 * t), without that batch -- five dense row-major [n_queries][n_targets] matrices; pos_a / len_a index the query, pos_b /
 * len_b the target; score and pos + len are seqalign_sw_score_cross's score and end_a / end_b; all five are 0 where no cell
 * is above 0.  The tiles are seqalign_sw_score_cross's with 20 result bytes per pair; queries of up to 512 columns run one
 * wave per (query, target) (the span kernel's cross form, recorded as "score_cross"), longer ones the span strips on explicit
 * pair lists ("score_strips").  The sweep costs what seqalign_sw_span_batch's costs, 3 - 4 x the score sweep.
 * Argument checks (before any device work: n_queries x n_targets overflowing uint64_t, NULL arguments, readable sets),
 * scoring admission (SEQALIGN_E_DOMAIN), empty sets (SEQALIGN_OK, nothing written) and SEQALIGN_E_UNKNOWN_PAIR ("query Q,
 * target T: ..." for the lowest q * n_targets + t) are seqalign_sw_score_cross's.  On an error the outputs are unspecified. */
int seqalign_sw_span_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                           const scoring_t *scoring, int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b,
                           uint32_t *out_len_a, uint32_t *out_len_b);
/* Statistics matrices: seqalign_nw_stats_batch's three outputs for every query against every target, [n_queries][n_targets]
 * each, the result of that call on the batch whose pair q * n_targets + t is (query q, target t) -- which is never built.
 * Queries of up to 512 columns run one wave per (query, target) on tiles of the two sets, 12 result bytes per pair; longer
 * queries run seqalign_nw_stats_batch's strips on their pairs.  Checks, admission, empty sets and the errors' "query Q, target
 * T: ..." for the lowest q * n_targets + t are seqalign_nw_score_cross's, SEQALIGN_E_TRACEBACK as in seqalign_nw_stats_batch.
 * There is no _cross_multi form. */
int seqalign_nw_stats_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                            const scoring_t *scoring, int32_t *out_score, uint32_t *out_matches, uint32_t *out_mismatches);
/* ---- NW gap-run counts: score and the gap opens of the global alignment, no traceback ---- */
/* For every pair, over the alignment seqalign_nw_batch returns for it -- the walk of alignment_reverse_move from the end
 * pick, tie order GAP_A, GAP_B, MATCH, not merely some optimal alignment:
 *   out_score[p]        byte for byte seqalign_nw_score_batch's;
 *   out_gap_runs_a[p]   the number of maximal runs of '-' in string a of that alignment;
 *   out_gap_runs_b[p]   the same count in string b.
 * BLAST's gapopen is their sum; an insertion directly against a deletion is two runs.  With seqalign_nw_stats_batch on the
 * same arguments this gives the tabular line of a global alignment -- pident, length, mismatch, gapopen, score -- in two
 * sweeps, nothing stored per cell.  A leading or trailing gap is a run like any other, free (no_start_gap_penalty,
 * no_end_gap_penalty) or not.  len_a = 0 < len_b gives (edge score, 1, 0), len_b = 0 < len_a (edge score, 0, 1), both empty
 * (0, 0, 0).  There is no limit on the lengths: a string has fewer than 2^31 columns, so the counts are full words beside the
 * sweep's "no walk" mark.
 *   Argument checks and their order, every error (SEQALIGN_E_DOMAIN, SEQALIGN_E_UNKNOWN_PAIR before SEQALIGN_E_TRACEBACK on
 * one pair), device bytes per pair, the 12 bytes home, chunking and launch kinds are seqalign_nw_stats_batch's.  Kernel:
 * sa_nw_gaps.hip.  Not here: _multi, _cross_multi, search, _submit, the command-line tools. */
int seqalign_nw_gaps_batch(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int32_t *out_score,
                           uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b);
/* Kernel time of seqalign_nw_gaps_batch (seq-align_amd/tools/nw_gaps_bench.py), as seqalign_nw_stats_time_ms */
int seqalign_nw_gaps_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int repeats,
                             float *ms_each);
/* Gap-run matrices: seqalign_nw_gaps_batch's three outputs for every query against every target, [n_queries][n_targets] each;
 * tiles, strips for long queries, checks, empty sets and errors are seqalign_nw_stats_cross's. */
int seqalign_nw_gaps_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                           const scoring_t *scoring, int32_t *out_score, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b);
/* seqalign_nw_gaps_batch over the banded NW matrices: out_score is seqalign_nw_score_banded's byte for byte, the two counts are
 * the '-' runs of seqalign_nw_align_banded's strings; where the unbanded alignment stays inside the band all three are
 * seqalign_nw_gaps_batch's.  The band, at most 512 diagonals, every check and its order, SEQALIGN_E_TRACEBACK for a pair with
 * no alignment inside the band, device bytes per pair, bytes home and launch records are seqalign_nw_stats_banded's.  Kernel:
 * sa_band_nw_frame.hpp by sa_band_nw_gaps.hip. */
int seqalign_nw_gaps_banded(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                            const uint32_t *band, int32_t *out_score, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b);
/* Timing hook (tools/nw_gaps_bench.py), as seqalign_nw_stats_band_time_ms for seqalign_nw_gaps_banded */
int seqalign_nw_gaps_band_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                  const uint32_t *band, int repeats, float *ms_each);
/* The wide form of seqalign_nw_gaps_banded: its argument list and contract word for word at any band width, score byte for
 * byte seqalign_nw_score_banded_wide's, the counts those of seqalign_nw_align_banded_wide's strings; strips, the option
 * band_strip_cols, device bytes and records are seqalign_nw_stats_banded_wide's.  A 200 kb pair in a band of 4 097 diagonals
 * gets its gapopen without any matrix.  No timing-hook, _multi, _submit or command-line form. */
int seqalign_nw_gaps_banded_wide(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring,
                                 const uint32_t *band, int32_t *out_score, uint32_t *out_gap_runs_a, uint32_t *out_gap_runs_b);
/* SW statistics matrices: seqalign_sw_stats_batch's seven outputs for every query against every target, [n_queries][n_targets]
 * each, the result of that call on the batch whose pair q * n_targets + t is (query q, target t) -- which is never built; pos_a
 * and len_a are in the query.  It runs on seqalign_sw_span_cross's tiles with 28 result bytes per pair: queries of up to 512
 * columns run one wave per (query, target), longer queries run seqalign_sw_stats_batch's strips on their pairs.  Every query and
 * every target must have at most SEQALIGN_SW_STATS_MAX_LEN letters (SEQALIGN_E_TOO_LARGE, "query Q: ..." / "target T: ...",
 * before the context is touched).  Checks, admission, empty sets and SEQALIGN_E_UNKNOWN_PAIR's "query Q, target T: ..." are
 * seqalign_sw_span_cross's.  There is no _cross_multi form. */
int seqalign_sw_stats_cross(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                            const scoring_t *scoring, int32_t *out_score, uint32_t *out_pos_a, uint32_t *out_pos_b,
                            uint32_t *out_len_a, uint32_t *out_len_b, uint32_t *out_matches, uint32_t *out_mismatches);
/* ... over several contexts: the query ranges of seqalign_sw_score_cross_multi; results exactly the single-context call's */
int seqalign_sw_span_cross_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                 const seqalign_seqset_t *targets, const scoring_t *scoring, int32_t *out_score,
                                 uint32_t *out_pos_a, uint32_t *out_pos_b, uint32_t *out_len_a, uint32_t *out_len_b);
typedef struct {
  uint32_t target;       /* index into the target set */
  int32_t score;
  uint32_t pos_a, pos_b, len_a, len_b; /* seqalign_sw_span_cross's at [q][target]; five zeros when score is 0 */
} seqalign_span_hit_t;   /* 24 bytes */
/* seqalign_sw_span_search: seqalign_sw_score_search with the hit's start beside its end.  n_hits[q] and the target and score
 * of every written slot are exactly that call's on the same arguments (order, min_score, k and every SEQALIGN_E_ARG case
 * unchanged); pos / len are seqalign_sw_span_cross's at [q][target], so pos + len is the score search's end_a / end_b.  A hit
 * of score 0 (selectable only with min_score <= 0) has five zeros.
 * Two stages: the score search as it is, then the span sweep on the selected hits alone -- for each the prefix pair
 * (query[0 : end_a], target[0 : end_b]), whose first hit is the full pair's, as one explicit pair list;
 * host memory for it grows with the hits, not with the sets.  The launches: "score_cross" / "score_select" (queries over
 * 1 024 columns: "score_strips"), then "score_rows" / "score_strips" for the prefixes.
 * SEQALIGN_E_UNKNOWN_PAIR is the score search's and named as it names it: every (query, target) is swept in full by the
 * first stage, so a failing pair outside the best k, or an unknown character past a selected hit's end cell, fails the call.
 * The result does not depend on tiling, chunk_bytes or the number of contexts. */
int seqalign_sw_span_search(seqalign_ctx_t *ctx, const seqalign_seqset_t *queries, const seqalign_seqset_t *targets,
                            const scoring_t *scoring, uint32_t k, int32_t min_score, seqalign_span_hit_t *hits,
                            uint32_t *n_hits);
int seqalign_sw_span_search_multi(seqalign_ctx_t *const *ctxs, int n_ctx, const seqalign_seqset_t *queries,
                                  const seqalign_seqset_t *targets, const scoring_t *scoring, uint32_t k, int32_t min_score,
                                  seqalign_span_hit_t *hits, uint32_t *n_hits);
/* Kernel time of the score-only call (seq-align_amd/tools/score_bench.py): the batch is packed and uploaded once (it must
 * fit one chunk), then its score kernels run `repeats` times, each launch between two HIP events: ms_each[r]. */
int seqalign_score_time_ms(seqalign_ctx_t *ctx, const seqalign_batch_t *batch, const scoring_t *scoring, int is_sw,
                           int repeats, float *ms_each);

/* ---- diagnostics ---------------------------------------------------------------- */
/* The host legs of seqalign_nw_batch's direction-byte path alone, no device involved: sizes, offsets and packing of the
 * sequences (pack_ms), then the expansion of synthetic all-MATCH moves into the caller's strings (expand_ms); averages
 * over `iterations`.  What one rank's CPU share sustains when N ranks do this at once (seq-align_amd/tools/host_scale.py). */
int seqalign_host_legs_nw(const seqalign_batch_t *batch, const uint64_t *str_off, char *out_a, char *out_b,
                          uint32_t *out_len, int iterations, double *pack_ms, double *expand_ms);

/* ---- misc ---------------------------------------------------------------------- */
/* The context's own stream (a hipStream_t as void*): what NULL means wherever a `stream` is passed.  For callers that
 * keep data in HBM and order their own work (events, copies) with the library's launches -- and a reason not to create
 * another stream for that: the runtime multiplexes the streams of one priority over four hardware queues, and every
 * further queue in use makes the host-level calls' own pipelines slower. */
void *seqalign_ctx_stream(seqalign_ctx_t *ctx);

/* Event pair on a stream for kernel timing (HIP events; bench.py). */
int seqalign_time_fill_ms(seqalign_ctx_t *ctx,
                          const seqalign_dev_scoring_t *scoring,
                          const seqalign_dev_batch_t *batch, int kernel,
                          void *stream, int repeats, float *ms_each);

#ifdef __cplusplus
}
#endif
#endif /* SEQALIGN_HIP_H */
