/* sa_kernels.h -- launch interface between sa_device.hip and the kernels.  HIP C++ only: every includer is a .hip file
 * (SaCrossParams and sa_pair_params below are templates, the latter __host__ __device__). */
#ifndef SA_KERNELS_H
#define SA_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "seqalign_hip.h"
extern "C" {
#include "sa_internal.h"   /* SA_F_* */
}

/* ---- the direction byte in its LOCAL form (round 6, second half) -----------------------------------------------------
 * The direction byte of sa_fill_dirs.hip answers, per state, "in which state does a walk that leaves this cell ARRIVE" -- for MATCH
 * and GAP_A that is a fact about the NEIGHBOUR (which of M / A / B is the maximum of the cell up-left; whether B >= M in the cell
 * above), which the fills carry over from the previous row and then convert, cell by cell, from comparison masks into two-bit
 * codes: select upon select -- 15-25 of a packed cell's ~115-165 issue cycles (profiles/r06/r06_local_dirs.txt).  A walk visits
 * ~170 of a pair's 22 801 cells.  So where ONLY tile walkers read the bytes (seqalign_nw_batch's moves path and the best-hit path:
 * every BASELINE config's host-level call but the multi-hit one) the fill stores each cell's OWN five
 * comparisons as five raw bits -- the sign bit of each saturating difference shifted into place, one v_lshrrev + one v_bitop3
 * per decision, no mask, no select, no carried tags -- and the walker reads the state it arrives in from the byte of the cell it
 * arrives at (it reads that byte anyway: it is the next step's):
 *     bit 0  GA  gap_a >= max(match, gap_b)        a walk that ARRIVES here by a MATCH move is in GAP_A if GA, else GAP_B if BM,
 *     bit 1  BM  gap_b >= match                     else MATCH (alignment.c:311-327's order); a GAP_A walk that opened its gap in
 *                                                   the cell below arrives in GAP_B if BM, else MATCH
 *     bit 2  CA  gap_a(above) + extend == gap_a     a GAP_A walk LEAVING this cell stays in GAP_A
 *     bit 3  FA  gap_a(left) + open + extend == gap_b   a GAP_B walk leaving this cell arrives in GAP_A,
 *     bit 4  FB  gap_b(left) + extend == gap_b          else GAP_B if FB, else MATCH
 *     bits 5 6 7 (Smith-Waterman)  this cell's match / gap_a / gap_b score is 0: a walk standing here in that state ends
 * The lane walkers look a cell AHEAD -- where a walk goes next must not wait for the byte of the cell it arrives at -- and keep the
 * older form (they walked launches of >= SA_WALK_TILE_MAX walks until the tile walks on the local form drew level with them at every
 * size: option trace_kernel = lane, or dirs_local = 0, brings them back); so do the multi-hit path's bytes, whose sweep routes
 * arrivals by them.  SaFillParams::dirs_local /
 * SaTraceParams::dirs_local say which form a launch writes / reads (option dirs_local = 0: the older form everywhere). */
#define SA_LD_GA 1u
#define SA_LD_BM 2u
#define SA_LD_CA 4u
#define SA_LD_FA 8u
#define SA_LD_FB 16u
#define SA_LD_END0 32u   /* << state */

/* Everything one fill launch needs; passed by value as the kernarg. */
/* ---- the direction bytes in BLOCKS (round 6) --------------------------------------------------------------------------
 * Where nobody but the walkers reads them -- seqalign_nw_batch's directions-only fills and the packed SW best-hit fill; not the
 * multi-hit path, whose sweep reads rows -- a pair's direction bytes are laid out in blocks of 8 rows x 16 columns = one 128-byte
 * line, block rows first:
 *     byte of cell (x, y)  at  ((y / 8) * nbx + x / 16) * 128 + (y % 8) * 16 + x % 16,      nbx = ceil((len_a + 1) / 16)
 * Row-major at a pitch of len_a + 1 bytes, a walk that climbs a row per step pulls in a new 128-byte line per step (measured:
 * 1.27 lines per step, 278 MB for C2's 10 000 walks, the walkers bound by exactly that: profiles/r06/r06_walkers.txt); in blocks a
 * diagonal walk stays 8-16 steps in a line.  The fills write a block row (8 rows: nbx x 128 contiguous bytes) at a time out of an
 * LDS buffer that is laid out the same way.  Rows of up to 512 columns (wider: row-major as before).  SA_DIRS_BLOCKED=0 (make exp)
 * builds the row-major form for an A/B. */
#ifndef SA_DIRS_BLOCKED
#define SA_DIRS_BLOCKED 1
#endif
static inline bool sa_dirs_blocked_shape(uint32_t max_len_a) { return SA_DIRS_BLOCKED != 0 && max_len_a + 1u <= 512u; }
static inline uint64_t sa_dirs_blocked_bytes(uint32_t len_a, uint32_t len_b) {   /* a multiple of 128 */
  return (uint64_t)((len_b + 8u) >> 3) * (uint64_t)((len_a + 16u) >> 4) * 128u;
}

struct SaFillParams {
  const uint8_t *arena;
  const uint64_t *off_a;
  const uint32_t *len_a;
  const uint64_t *off_b;
  const uint32_t *len_b;
  const uint64_t *mat_off;
  int32_t *M, *A, *B;
  uint64_t *status;
  const uint16_t *code;   /* [256] raw char -> folded char | class << 8 */
  const int32_t *table;   /* [K*K] */
  uint32_t n_pairs;
  uint32_t K;
  int32_t gap_open, open1, ext, floor, gen_eq, gen_ne;
  uint32_t flags;         /* SA_F_* (sa_internal.h) */
  /* optional (stream kernel, SW): the best match_scores cell per pair in the reference's
   * hit order (score desc, column asc, index asc), as sa_reduce.hip reports it -- saves the
   * separate pass over match_scores when only the best hit is wanted */
  int32_t *best_score;
  uint64_t *best_index;
  /* optional (stream kernel, SW): what the multi-hit path needs to know about match_scores before it sweeps the
   * matrices backwards (sa_sw_sweep.hip) -- whether any cell has score >= max(cand_min[pair], 1) (the candidates of
   * smith_waterman.c:152-156; cand_count != 0) and bounds of where they are: cand_box[4*pair..] = first row, last row,
   * a column at or below the lowest, a column at or above the highest candidate column. */
  const int32_t *cand_min;
  uint32_t *cand_count;
  uint32_t *cand_box;
  uint32_t *cand_rows;          /* the multi-hit path's scratch arena (SaSweepParams::hit_keys) as uint32: pair p's part starts
                                    with its rows' candidate columns -- lowest / highest per row, rows 0..len_b (lo > hi: none) */
  const uint64_t *cand_rows_off; /* [n] where pair p's part starts, in uint64 (SaSweepParams::hit_off)                    */
  /* launch tuning (host side only; the context's options, sa_ctx.hpp SaOptions): 0 = the launcher's own choice */
  uint32_t tune_cpl, tune_wpb, tune_lds_pad;
  uint32_t tune_quad = 0;   /* host side only: the packed fills with four pairs per wave: 0 = by shape and size, 1 = never, 2 = whenever the shape allows (option quad) */
  /* != 0: every pair of the launch has the same len_a and len_b and pair k's cells start at mat_off[0] + k * uniform_stride
   * (>= its cell count); the packed two-pairs-per-wave fills (sa_fill_dirs_x2.hip) need a multiple of 256 */
  uint64_t uniform_stride;
  const uint32_t *pair_list;    /* optional (the direction fills of seqalign_nw_batch): the launch takes pairs pair_list[0 .. n_pairs)
                                   of the descriptor arrays instead of pairs 0 .. n_pairs -- a chunk whose pairs are MOSTLY of one
                                   shape goes through the packed kernel with the list of those, the others through the one-pair
                                   kernel with the list of the rest */
  int32_t table_abs_max;        /* host side only: the largest |entry| of the K x K table (0 for K <= 1): the packed fills' int16 bound */
  uint32_t dirs_local = 0;      /* host side only: the NW / best-hit direction fills write the LOCAL form of the byte (above) */
};

/* How the multi-hit path packs a match_scores cell into a 64-bit key whose ascending order IS the reference's hit
 * order (score desc, column asc, then cell index = row asc; smith_waterman.c:71-86):
 *     key = (cap - score) << (row_bits + col_bits) | column << row_bits | row
 * cap = an upper bound of every score of the chunk; row_bits + col_bits + score_bits <= 63. */
struct SaKeyLayout {
  int32_t cap;
  uint32_t row_bits, col_bits, score_bits;
};

struct SaReduceParams {
  const uint32_t *len_a, *len_b;
  const uint64_t *mat_off;
  const int32_t *M;
  int32_t min_score;
  int32_t *best_score;
  uint64_t *best_index;
  uint32_t *cand_count;
  const uint64_t *cand_off;
  const uint32_t *cand_cap;
  uint32_t *cand_index;
  int32_t *cand_score;
  uint32_t n_pairs;
  uint32_t slices;   /* > 1 (best cell only, few long pairs): that many waves per pair (sa_reduce.hip) */
  uint32_t tune_depth; /* host side only: 0 = by the launch's size, 4 / 8 = KiB a wave loads per step (option reduce_depth) */
};

/* candidate count and bounding box per pair, as the stream fill (SA_STREAM_CAND) or sa_launch_sw_box leaves them */
struct SaCandBox {
  uint32_t *cand_count;       /* [n]                                                       */
  uint32_t *cand_box;         /* [4n] rmin, rmax, cmin, cmax                               */
  uint32_t *cand_rows;        /* the multi-hit path's scratch arena, as uint32 (SaFillParams::cand_rows) */
  const uint64_t *hit_off;    /* [n + 1] where pair p's part of it starts, in uint64       */
  const int32_t *cand_min;    /* [n] per-pair min_score                                    */
  uint8_t *dirs;              /* optional: room for one byte per cell (same cell offsets as the matrices).  If the batch is in
                                 sa_fill_dirs.hip's domain the fill writes match_scores + directions there INSTEAD of the three
                                 matrices and sets *dirs_used (gap_a / gap_b are then not written at all)                     */
  bool *dirs_used;
  bool best_only;             /* dirs + dirs_used as above, but for the best-hit path: no candidate outputs (the cand_* members
                                 are NULL), the fill writes ONLY the direction bytes and reports the best cell through the
                                 best_score / best_index arguments (sa_fill_dirs_x2.hip: fill_sw_best_x2_kernel); the chunk's
                                 three matrices are not even allocated */
  uint64_t uniform_stride;    /* != 0: the chunk's layout is SaFillParams::uniform_stride's (every pair the same shape, cells
                                 k * uniform_stride apart): the packed two-pairs-per-wave fill may take it (sa_fill_dirs_x2.hip) */
  const uint32_t *pair_list;  /* != NULL (ragged chunk, every pair's cells on a multiple of 256, uniform_stride = 256): the packed fill takes
                                 list_count / 2 waves, wave u the pairs pair_list[2u], pair_list[2u + 1] of the descriptor arrays -- equal in
                                 shape, or the same pair twice (it has the wave to itself)                                               */
  uint32_t list_count;
  bool dirs_local;            /* best_only: the fill writes the LOCAL form of the direction byte (tile walkers behind it) */
};

/* SW multi-hit enumeration: the reverse sweep (sa_sw_sweep.hip) */
struct SaSweepParams {
  const uint8_t *arena;
  const uint64_t *off_a;
  const uint32_t *len_a;
  const uint64_t *off_b;
  const uint32_t *len_b;
  const uint64_t *mat_off;
  const int32_t *M, *A, *B;      /* OVER-READ (sw_sweep_dirs_ev_kernel, branchless row loads): up to CPL * 4 <= 64 bytes of M and
                                    CPL + 3 <= 19 bytes of `dirs` BEHIND the last pair's last cell are loaded (never used): the
                                    caller's arenas must extend that far (sa_host::reserve_arenas and the dirs buffers add 4 KiB) */
  const uint16_t *code;
  const int32_t *table;
  const uint32_t *cand_count;    /* [n]                                                              */
  const uint32_t *cand_box;      /* [4n]                                                             */
  const int32_t *min_score;      /* [n]                                                              */
  unsigned long long *hit_keys;  /* scratch arena; pair p's part is elements [hit_off[p], hit_off[p + 1]): first len_b + 1
                                    elements = its rows' candidate columns (in: the fill / sa_launch_sw_box), then (out) its
                                    hits' keys: ascending when hit_count <= 64, else in the order the sweep met them
                                    (SA_SWEEP_UNSORTED)                                                           */
  const uint64_t *hit_off;       /* [n + 1]; room for hits: a hit owns at least ceil(min_score / best move) + 1 cells  */
  uint32_t *hit_count;           /* [n] every hit of the pair (no max_hits here)                      */
  uint32_t *status;              /* [n] 0, SEQALIGN_E_* of a walk (see err_key), | SA_SWEEP_UNSORTED   */
  unsigned long long *err_key;   /* [n] key of the first (lowest) walk that met the error             */
                                 /* (strips: the caller zeroes hit_count / status and sets err_key to ~0)            */
  uint32_t lds_columns;          /* one wave per pair, wide rows: the winners of two rows live in LDS, sized for this
                                    many columns (>= every pair's len_a + 1)                                         */
  /* one wave per strip of strip_columns columns (few wide pairs; strip_progress != NULL selects it): */
  uint32_t *strip_progress;      /* [2 * sa_sweep_strip_blocks() + 1] zeroed: per (pair, strip) rows done | end, then
                                    the ticket counter                                                               */
  uint32_t strip_columns;        /* 64, 128 or 256                                                                   */
  uint32_t strip_interval;       /* rows between two publications of a strip's progress: 16 or 64                    */
  uint32_t strips_per_pair;      /* sa_sweep_strips_per_pair(max_len_a, strip_columns)                               */
  unsigned long long *bnd;       /* per pair, row (counted from the box's last row) and strip: the winner of the strip's
                                    first column, 2 uint64; pair p at 2 * row_off[p] * strips_per_pair               */
  const uint64_t *row_off;       /* [n] prefix of len_b + 1                                                          */
  uint32_t n_pairs, K;
  int32_t open1, ext, gen_eq, gen_ne;
  uint32_t flags;
  uint32_t max_len_a;            /* of the chunk: picks the kernel                                    */
  uint32_t max_len_b;            /* of the chunk (0: unknown): with max_len_a the radices of the sweep's mixed-radix 32-bit word  */
  SaKeyLayout layout;
  unsigned long long *trace;     /* optional [8n]: cycles, rows, active row segments, rounds, cycles in active segments (option sweep_trace) */
  uint32_t tune_ev;              /* host side only: the direction-byte sweep's second form (walks as key << 2 | state words; option sweep_ev) */
  uint32_t tune_cpl;             /* host side only: 1, 2, 4 forces the LDS form with segments of 64 * that many columns (option sweep_cpl) */
  const uint8_t *dirs;           /* != NULL: the matrices were filled by sa_fill_dirs.hip -- M holds match_scores, dirs one byte
                                    of directions per cell (same cell offsets), A / B are not used                           */
};
#define SA_SWEEP_UNSORTED 0x80000000u
#define SA_SWEEP_OVERFLOW 0x40000000u   /* more hits than the pair's part of the arena holds (cannot happen: see hit_off) */
/* widest pair (columns) whose two rows of records fit LDS (12 B per column and row with 64-bit keys) */
#define SA_SWEEP_LDS_COLUMNS 2048u
uint32_t sa_sweep_strips_per_pair(uint32_t max_len_a, uint32_t strip_columns);
uint32_t sa_sweep_strip_blocks(uint32_t n_pairs, uint32_t max_len_a, uint32_t strip_columns);

struct SaTraceParams {
  const uint8_t *arena;
  const uint64_t *off_a;
  const uint32_t *len_a;
  const uint64_t *off_b;
  const uint32_t *len_b;
  const uint64_t *mat_off;
  const int32_t *M, *A, *B;
  const uint16_t *code;
  const int32_t *table;
  const uint64_t *str_off;
  char *out_a, *out_b;
  uint32_t *out_head, *out_len;
  int32_t *out_score;
  uint32_t *trace_status;
  /* pipelined host-level calls (sa_batch.hip): when out_meta4 != NULL the four per-walk words go there instead,
   * interleaved -- head, len, score, status of walk w at out_meta4[4w..] -- so that one sub-batch's results are ONE
   * contiguous D2H; fill_status (optional, [n] per pair): a fill status != ~0 (a character pair without a score,
   * alignment_scoring.c:178-181) becomes the walk's status SEQALIGN_E_UNKNOWN_PAIR, which saves copying the fill's
   * status words back separately */
  uint32_t *out_meta4;
  const uint64_t *fill_status;
  const uint64_t *start_index; /* SW: end cell of the hit per pair; NULL = NW        */
  uint32_t *out_pos;           /* SW: [4*n] pos_a, pos_b, len_a, len_b               */
  /* SW multi-hit path: n_pairs WALKS, walk w = hit walker_rank[w] of pair walker_pair[w], ending at the cell packed in
   * hit_keys[mat_off[pair] + rank] (layout); str_off and every out_* array are indexed by the walk */
  const uint32_t *walker_pair, *walker_rank;
  const unsigned long long *hit_keys;
  const uint64_t *hit_off;     /* (SaSweepParams::hit_off: pair p's keys start at hit_off[p] + len_b + 1) */
  SaKeyLayout layout;
  uint32_t n_pairs, K;
  int32_t open1, ext, gen_eq, gen_ne;
  uint32_t flags;
  uint32_t tune_walker;        /* host side only: 0 = by batch shape, 1 = one lane per walk, 2 = one wave per walk (option trace_kernel) */
  uint32_t dirs_blocked;       /* `dirs` is laid out in blocks of 8 x 16 cells (above) instead of row-major at pitch len_a + 1 */
  uint32_t tune_group;         /* host side only: the tile walker on moves: 0 / 4 = four walks per wave in lockstep, 8 = eight, 1 = one (option walk_group) */
  uint32_t tune_tile;          /* host side only: the local tile walker's tile edge: 32 or 64 bytes; 0 = 32 for NW walks, 64 for SW ones (option walk_tile) */
  uint32_t tune_stage;         /* host side only: the local tile walker writes a wave's moves as one run out of LDS (option walk_stage) */
  uint32_t dirs_local;         /* `dirs` holds the LOCAL form of the direction byte (above): tile walkers on moves only */
  const uint8_t *dirs;         /* SW multi-hit path behind sa_fill_dirs.hip: walks follow the direction bytes (hit_keys != NULL) */
  const int32_t *nw_score;     /* NW behind the directions-only fill (dirs != NULL): per pair the end cell's score ...            */
  const uint64_t *nw_state;    /* ... and the matrix the walk starts in (0 MATCH, 1 GAP_A, 2 GAP_B)                                */
  const int32_t *start_score;  /* SW walks on direction bytes from start_index (the best-hit path behind fill_sw_best_x2_kernel, which
                                  writes no match_scores): the start cell's score                                                  */
  /* walks on direction bytes that send home MOVES instead of strings (host/sa_moves.c): per walked column one bit "gap in
   * seq_a" (the walk stood in GAP_A) and one bit "gap in seq_b", forward column order, right-aligned in the walk's slot --
   * walk w owns words [2 ((str_off[w] >> 5) + w), + 2 nw) of `moves`, nw = (len_a + len_b + 31) >> 5: plane A, then plane B
   * (str_off is the prefix of len_a + len_b, so the slots do not overlap); out_a / out_b / out_meta4 are not used, the two
   * words of walk w go to out_meta2[2w..]: score, then the number of walked columns -- or 0xFFFFFFF0 | SEQALIGN_E_* .
   * SW walks also need out_pos for nothing: the host derives the hit's position from the planes (sa_expand_sw_moves). */
  uint32_t *moves;
  uint32_t stage_words = 0;    /* >= (len_a + len_b + 31) >> 5 of every walk of the launch (0 = unknown): the one-lane-per-walk kernel keeps a walk's
                                  finished words in LDS until it is over (up to 96 words: 3 040 columns) */
  uint32_t *out_meta2;
  /* SW walks that send home moves: out_meta4[4w..] = score, walked columns, end cell x, y.  walks_per_pair = k > 0: the launch has
   * k walks per pair, walk w = hit w % k of pair w / k (its key in hit_keys), in the slot 2 k ((str_off[pair] >> 5) + pair) +
   * 2 (w % k) nw -- str_off then indexed by PAIR -- and walks beyond hit_count[pair], or of a pair with sweep_status != 0,
   * return without a trace: the launch can be enqueued before anybody has seen the sweep's counts */
  uint32_t walks_per_pair;
  const uint32_t *hit_count, *sweep_status;
};
/* direction-byte walks: one wave per walk (LDS tiles) below this many walks per launch, one lane per walk from there on (sa_traceback.hip) */
#define SA_WALK_TILE_MAX 24576u
#define SA_MOVES_ERR 0xFFFFFFF0u

/* ---- which kernels a call launched (seqalign_ctx_last_call_info, include/seqalign_hip.h: SEQALIGN_K_*) ------------------
 * Every launcher below reports what it launches and for how many pairs / walks to the calling thread's recorder
 * (sa_device.hip), which the C-ABI entry points point at their context for the duration of the call. */
void sa_record_launch(int kind, uint64_t items);

/* substitution lookup flavour */
enum { SA_SUBST_SIMPLE = 0, SA_SUBST_LDS = 1, SA_SUBST_GLOBAL = 2 };
#define SA_LDS_TABLE_MAX_K 64

/* ---- the DOMAINS of the direction-byte fills: pure functions of (flattened scoring, shape) ---------------------------
 * Which scorings and shapes a kernel family takes is a property of the scoring's numbers and the pairs' lengths alone; the
 * launchers add what depends on the launch (output pointers present, block-aligned), and the host-level entry points ask the
 * same functions BEFORE they lay a chunk out (sa_device.hip: *_applicable) -- from the flattened scoring, no launch needed. */
struct SaScoringTraits {
  uint32_t flags, K;
  int32_t gap_open, open1, ext, gen_eq, gen_ne, table_abs_max;
};
inline SaScoringTraits sa_traits_of(const SaFillParams &p) {
  return SaScoringTraits{p.flags, p.K, p.gap_open, p.open1, p.ext, p.gen_eq, p.gen_ne, p.table_abs_max};
}
/* the row sweeps' GENERAL path (free / forbidden gaps, sentinel scores, gap_open > 0): none of the direction fills takes it */
inline bool sa_scoring_needs_general(const SaScoringTraits &t) {
  return (t.flags & (SA_F_NO_END_GAP | SA_F_NO_GAPS_A | SA_F_NO_GAPS_B | SA_F_HAS_SENTINEL)) || t.open1 > t.ext;
}
/* rows the direction fills keep in one wave's registers: 16 columns per lane (round 5; 8 before).  The SW sweep behind them
 * keeps a row in registers too: up to 512 columns in either of its forms, 513 .. 1 024 in the one-word form only
 * (sw_sweep_dirs_ev_kernel, keys of <= 62 bits) -- the caller (sa_batch_sw.hip) offers a direction arena only when that holds */
/* NW, directions only: no flag at all, no sentinel, gap_open <= 0, gap_extend <= 0, a table that fits LDS */
inline bool sa_domain_nw_dirs_row(uint32_t max_len_a) { return max_len_a + 1 <= 16 * 64; }
inline bool sa_domain_nw_dirs(const SaScoringTraits &t, uint32_t max_len_a) {
  return t.flags == 0 && !sa_scoring_needs_general(t) && t.K <= SA_LDS_TABLE_MAX_K && t.ext <= 0 && sa_domain_nw_dirs_row(max_len_a);
}
/* SW, match_scores + directions / directions + best cell: the same without the start-gap / mismatch flags */
inline bool sa_domain_sw_dirs(const SaScoringTraits &t, uint32_t max_len_a) {
  return (t.flags & SA_F_IS_SW) && !sa_scoring_needs_general(t) && !(t.flags & (SA_F_NO_START_GAP | SA_F_NO_MISMATCH)) &&
         t.K <= SA_LDS_TABLE_MAX_K && t.ext <= 0 && sa_domain_nw_dirs_row(max_len_a);
}
/* two pairs per wave in packed int16: every score the recurrence can produce on pairs up to max_len_a x max_len_b, de-trended
 * or not, stays inside int16 */
inline bool sa_domain_x2_scores_fit(const SaScoringTraits &t, uint32_t max_len_a, uint32_t max_len_b) {
  auto mag = [](int64_t v) { return v < 0 ? -v : v; };
  int64_t pen = mag(t.gen_eq) > mag(t.gen_ne) ? mag(t.gen_eq) : mag(t.gen_ne);
  if (mag(t.open1) > pen) pen = mag(t.open1);
  if (mag(t.ext) > pen) pen = mag(t.ext);
  if (mag(t.gap_open) + mag(t.ext) > pen) pen = mag(t.gap_open) + mag(t.ext);
  if (t.K > 1 && (int64_t)t.table_abs_max > pen) pen = t.table_abs_max;
  return ((int64_t)max_len_a + max_len_b + 2) * pen + ((int64_t)max_len_a + 1) * mag(t.ext) <= 30000;
}
/* ... and for the packed NW fills (round 6), which keep every value V of cell (g, j) as V - (g + j) gap_extend (the recurrence of gap_a
 * loses its "+ extend", gap_b's scan its re-trend: two packed adds per cell): |V'| <= (la + lb + 2) (pen + |extend|) */
inline bool sa_domain_nw_x2_scores_fit(const SaScoringTraits &t, uint32_t max_len_a, uint32_t max_len_b) {
  auto mag = [](int64_t v) { return v < 0 ? -v : v; };
  int64_t pen = mag(t.gen_eq) > mag(t.gen_ne) ? mag(t.gen_eq) : mag(t.gen_ne);
  if (mag(t.open1) > pen) pen = mag(t.open1);
  if (mag(t.ext) > pen) pen = mag(t.ext);
  if (mag(t.gap_open) + mag(t.ext) > pen) pen = mag(t.gap_open) + mag(t.ext);
  if (t.K > 1 && (int64_t)t.table_abs_max > pen) pen = t.table_abs_max;
  return ((int64_t)max_len_a + max_len_b + 2) * (pen + mag(t.ext)) <= 30000;
}
inline bool sa_domain_nw_dirs_x2(const SaScoringTraits &t, uint32_t la, uint32_t lb) {
  return sa_domain_nw_dirs(t, la) && sa_domain_nw_x2_scores_fit(t, la, lb);
}
inline bool sa_domain_sw_dirs_x2(const SaScoringTraits &t, uint32_t la, uint32_t lb) {
  return sa_domain_sw_dirs(t, la) && sa_domain_x2_scores_fit(t, la, lb);
}
/* (the best-hit fill has no sweep behind it: like the NW fill it takes rows up to 1 024 columns -- round 5) */
inline bool sa_domain_sw_best_x2(const SaScoringTraits &t, uint32_t la, uint32_t lb) {
  return (t.flags & SA_F_IS_SW) && !sa_scoring_needs_general(t) && !(t.flags & (SA_F_NO_START_GAP | SA_F_NO_MISMATCH)) &&
         t.K <= SA_LDS_TABLE_MAX_K && t.ext <= 0 && sa_domain_nw_dirs_row(la) && lb < 32768 && sa_domain_x2_scores_fit(t, la, lb);
}

/* ---- the int32 domain of the row sweeps (include/seqalign_hip.h, SEQALIGN_E_DOMAIN) --------------------------------------
 * Every kernel that sweeps a row de-trends gap_b (sa_rowsweep.hpp): it adds to a cell up to `cols` times |gap_extend|, a sum the
 * reference never forms, and takes a maximum before it takes the trend back -- so that sum must fit int32, or a cell that
 * should win the maximum loses it.  No cell of a pair of up to la x lb letters holds more than
 *     bound = max(n P + (la + lb - 2 n) G, (la + lb) G),   n = min(la, lb),
 * P = the largest substitution score above 0, G = the largest of gap_open + gap_extend and gap_extend above 0 (an alignment
 * has at most n columns of two letters, and every other column is a gap column).  cols: with gap_extend <= 0 the trend grows
 * with the position inside the frame, below the row's la + 1 columns (SA_FRAMES_BAND: below the band's at most la + lb + 1
 * diagonals) and below the frame's width; with gap_extend > 0 it is taken from the frame's far end and is the frame's width
 * whatever the row.  Frames are 1 024 columns at most, 4 096 where a call that fills whole matrices (SA_FRAMES_FILL) may take
 * the workgroup fill (sa_fill_wgstream.hip: rows of 1 025 columns and more).  Admitted: bound + cols |gap_extend| <= INT32_MAX.
 * The same bound keeps the kernels' products g * gap_extend inside int32. */
enum SaFrames { SA_FRAMES_FILL = 0, SA_FRAMES_ROWS = 1, SA_FRAMES_BAND = 2 };
struct SaMagnitude { uint64_t bound, cols, ext_abs; };   /* all three saturate at 2^62 */
inline SaMagnitude sa_domain_magnitude(int32_t pos_max, int32_t open1, int32_t ext, uint64_t la, uint64_t lb, SaFrames frames) {
  typedef unsigned __int128 u128;
  const u128 sat = (u128)1 << 62;
  const u128 P = pos_max > 0 ? (u128)pos_max : 0, G = (u128)(open1 > ext ? (open1 > 0 ? open1 : 0) : (ext > 0 ? ext : 0));
  const u128 n = la < lb ? la : lb, all = (u128)la + lb;
  const u128 mixed = n * P + (all - 2 * n) * G, gaps = all * G;
  const u128 bound = mixed > gaps ? mixed : gaps;
  const uint64_t cap = (frames == SA_FRAMES_FILL && la >= 1024) ? 4096 : 1024;
  const u128 reach = frames == SA_FRAMES_BAND ? all + 1 : (u128)la + 1;
  const uint64_t cols = ext > 0 || reach > cap ? cap : (uint64_t)reach;
  return SaMagnitude{(uint64_t)(bound < sat ? bound : sat), cols, ext < 0 ? (uint64_t)(-(int64_t)ext) : (uint64_t)ext};
}
inline bool sa_domain_magnitude_fits(const SaMagnitude &m) { return m.bound + m.cols * m.ext_abs <= (uint64_t)INT32_MAX; }

/* returns hipSuccess or the launch error; never synchronises */
hipError_t sa_launch_fill_wavefront(const SaFillParams &p, uint32_t max_len_a,
                                    hipStream_t stream);
hipError_t sa_launch_fill_rowscan(const SaFillParams &p, uint32_t max_len_a,
                                  hipStream_t stream);
/* LDS-ring stream writer; only when sa_stream_kernel_applicable() */
bool sa_stream_kernel_applicable(const SaFillParams &p, uint32_t max_len_a);
hipError_t sa_launch_fill_stream(const SaFillParams &p, uint32_t max_len_a,
                                 hipStream_t stream);
/* whether sa_launch_fill_stream would also report the candidates' count and box (p.cand_*) */
bool sa_stream_kernel_emits_candidates(const SaFillParams &p, uint32_t max_len_a);
/* whether sa_launch_fill_stream would also fill p.best_score / p.best_index */
bool sa_stream_kernel_reports_best(const SaFillParams &p, uint32_t max_len_a, uint32_t max_len_b);
/* few long pairs: the column strips of a pair as a pipeline of waves (any len_a);
 * progress = 8 * ceil(n_pairs / 8) * sa_fill_strips_per_pair(max_len_a) + 1 uint32 of scratch (the last one is
 * the ticket counter, sa_fill_strips.hip) */
uint32_t sa_fill_strips_per_pair(uint32_t max_len_a);
hipError_t sa_launch_fill_strips(const SaFillParams &p, uint32_t max_len_a, uint32_t *progress, hipStream_t stream);

/* ---- score only (sa_score.hip): the row sweep of every fill, nothing stored per cell --------------------------------------
 * Pair k of a launch: score[k] (NW: max of match / gap_a / gap_b at (len_a, len_b); SW: the best match_scores cell in hit
 * order) and, SW only, that cell's 1-based coordinates end_a[k] = column i, end_b[k] = row j (0, 0 when no cell is above 0);
 * f.status[k] = the first cell without a score (~0: none); *err_flag |= 1 when any pair of the launch has one.
 * Rows of up to SA_SCORE_ROW_MAX columns: one wave per pair.  Wider: strips of 512 columns, one wave each, handing their last
 * column over through `handoff` (no cap on len_a x len_b). */
#define SA_SCORE_ROW_MAX 1024u
struct SaScoreParams {
  SaFillParams f;               /* sequences, descriptors, scoring, status; the matrix pointers are unused              */
  int32_t *score;               /* [n]                                                                                 */
  uint32_t *end_a, *end_b;      /* [n] (SW)                                                                            */
  uint32_t *err_flag;           /* one word, zeroed by the caller                                                      */
  /* strips only: */
  uint32_t *progress;           /* [8 * ceil(n / 8) * strips_per_pair + 1] zeroed: rows done per (pair, strip), then the
                                   ticket counter                                                                       */
  int32_t *handoff;             /* pair k, strip s < last: rows 0 .. len_b of {max(M, A), B} of the strip's last column
                                   at 2 * (handoff_off[k] + s * (len_b + 1))                                            */
  const uint64_t *handoff_off;  /* [n]                                                                                 */
  uint32_t *strip_best;         /* [4 * progress words] SW: the best cell of strips 0 .. s (score, column, row)        */
  uint32_t strips_per_pair;
};
/* One buffer holds `words` progress words, the ticket counter behind them and then, 16-byte aligned, strip_best. */
static inline uint64_t sa_strip_best_word(uint64_t words) { return (words + 1 + 3) & ~(uint64_t)3; }
static inline uint64_t sa_strip_progress_bytes(uint64_t words) { return 4 * sa_strip_best_word(words) + 16 * words; }
uint32_t sa_score_strips_per_pair(uint32_t max_len_a);
/* every pair of the launch has len_a <= SA_SCORE_ROW_MAX; max_len_a picks the columns per lane */
hipError_t sa_launch_score_rows(const SaScoreParams &p, uint32_t max_len_a, bool is_sw, hipStream_t stream);
/* the caller zeroed progress (and err_flag) and set status to ~0 */
hipError_t sa_launch_score_strips(const SaScoreParams &p, bool is_sw, hipStream_t stream);
/* The one-wave kernels' row classes: columns per lane 1 .. 16 in these steps, one launch per class; a row of len_a columns
 * takes the narrowest class that holds it (SA_SCORE_ROW_CLASSES: wider than SA_SCORE_ROW_MAX, the strips kernel). */
#define SA_SCORE_ROW_CLASSES 9
static inline int sa_score_row_class(uint32_t len_a) {
  static const uint32_t cpl[SA_SCORE_ROW_CLASSES] = {1, 2, 3, 4, 5, 6, 8, 12, 16};
  if (len_a > SA_SCORE_ROW_MAX) return SA_SCORE_ROW_CLASSES;
  const uint32_t need = (len_a + 63) / 64;
  int c = 0;
  while (cpl[c] < need) ++c;
  return c;
}
/* ---- SW hit spans (sa_span.hip): sa_score.hip's SW sweep with the start of the best hit carried beside the scores -------
 * Pair k of a launch: score[k], pos_a[k], pos_b[k], len_a[k], len_b[k] = the fields of the reference's first hit (all 0 when
 * no cell is above 0); f.status / err_flag as SaScoreParams.  Rows of up to SA_SPAN_ROW_MAX columns: one wave per pair
 * (columns per lane 1 .. 6 and 8).  Wider: strips of 512 columns handing over SA_SPAN_HANDOFF_BYTES per row. */
#define SA_SPAN_ROW_MAX 512u
#define SA_SPAN_HANDOFF_BYTES 32u
#define SA_SPAN_BEST_BYTES 32u
struct SaSpanParams {
  SaFillParams f;
  int32_t *score;                                 /* [n]                                                              */
  uint32_t *pos_a, *pos_b, *len_a, *len_b;        /* [n]                                                              */
  uint32_t *err_flag;                             /* one word, zeroed by the caller                                   */
  /* strips only: */
  uint32_t *progress;           /* as SaScoreParams                                                                    */
  int32_t *handoff;             /* pair k, strip s < last: rows 0 .. len_b, SA_SPAN_HANDOFF_BYTES each, at
                                   SA_SPAN_HANDOFF_BYTES * (handoff_off[k] + s * (len_b + 1))                           */
  const uint64_t *handoff_off;  /* [n], in rows                                                                        */
  uint32_t *strip_best;         /* SA_SPAN_BEST_BYTES per progress word                                                */
  uint32_t strips_per_pair;
};
static inline uint64_t sa_span_progress_bytes(uint64_t words) { return 4 * sa_strip_best_word(words) + SA_SPAN_BEST_BYTES * words; }
uint32_t sa_span_strips_per_pair(uint32_t max_len_a);
/* every pair of the launch has len_a <= SA_SPAN_ROW_MAX; max_len_a picks the columns per lane */
hipError_t sa_launch_span_rows(const SaSpanParams &p, uint32_t max_len_a, hipStream_t stream);
/* the caller zeroed progress (and err_flag) and set status to ~0 */
hipError_t sa_launch_span_strips(const SaSpanParams &p, hipStream_t stream);
/* the one-wave span kernels' row classes, as sa_score_row_class (SA_SPAN_ROW_CLASSES: the strips kernel) */
#define SA_SPAN_ROW_CLASSES 7
static inline int sa_span_row_class(uint32_t len_a) {
  static const uint32_t cpl[SA_SPAN_ROW_CLASSES] = {1, 2, 3, 4, 5, 6, 8};
  if (len_a > SA_SPAN_ROW_MAX) return SA_SPAN_ROW_CLASSES;
  const uint32_t need = (len_a + 63) / 64;
  int c = 0;
  while (cpl[c] < need) ++c;
  return c;
}
/* Two sets instead of a pair list (the *_cross calls): one launch per row class of the queries, one wave per (query, target),
 * for the one-wave kernel of every family -- P is its parameter block (SaScoreParams, SaSpanParams, SaStatsParams,
 * SaSwStatsParams).  s.f.off_a / s.f.len_a: the tile's queries, s.f.off_b / s.f.len_b: its targets, both into s.f.arena;
 * s.f.n_pairs, s.f.status and the strips fields of s are unused.  The result arrays of s: [q * n_t + t] for every query q of
 * the tile; s.err_flag |= 1 when a pair has a cell without a score. */
template <class P>
struct SaCrossParams {
  P s;
  const uint32_t *q_list;       /* [nq] the class's queries (indices into s.f.off_a / s.f.len_a)                       */
  const uint32_t *t_order;      /* [n_t] every target of the tile, longest first (indices into s.f.off_b / s.f.len_b)   */
  uint32_t nq, n_t;
  uint32_t n_waves;             /* nq * n_t                                                                            */
  unsigned long long *err_pair; /* min of q * n_t + t over the failing pairs; the caller set it to ~0                  */
};
/* a family's parameter block inside either form */
template <class P> __host__ __device__ inline const P &sa_pair_params(const P &p) { return p; }
template <class P> __host__ __device__ inline const P &sa_pair_params(const SaCrossParams<P> &p) { return p.s; }
using SaScoreCrossParams = SaCrossParams<SaScoreParams>;
using SaSpanCrossParams = SaCrossParams<SaSpanParams>;
/* every query of the class has len_a <= max_len_a <= SA_SCORE_ROW_MAX */
hipError_t sa_launch_score_cross(const SaScoreCrossParams &p, uint32_t max_len_a, bool is_sw, hipStream_t stream);
/* SW hit spans over two sets (seqalign_sw_span_cross): the CROSS form of sa_span.hip's one-wave kernel;
 * every query of the class has len_a <= max_len_a <= SA_SPAN_ROW_MAX; recorded as "score_cross" (items: waves) */
hipError_t sa_launch_span_cross(const SaSpanCrossParams &p, uint32_t max_len_a, hipStream_t stream);
/* ---- NW alignment statistics (seqalign_nw_stats_batch / _cross, sa_nw_stats.hip): sa_score.hip's NW sweep with two counters
 * carried beside the three values of a cell.  Pair k of a launch: score[k] = SaScoreParams' NW score,
 * matches[k] / mismatches[k] = the columns of the alignment seqalign_nw_batch returns that hold two equal / two different
 * letters (after the scoring's case folding); bit 31 of mismatches[k] (SA_STATS_NO_WALK) = the end pick's state has no walk
 * (SEQALIGN_E_TRACEBACK).  f.status / err_flag as SaScoreParams.  Row classes, strips, hand-off bytes and the layout of
 * `progress` are the span kernels' (SA_SPAN_ROW_MAX, sa_span_row_class, sa_span_strips_per_pair, SA_SPAN_HANDOFF_BYTES);
 * there is no best cell, so nothing follows the ticket counter. */
#define SA_STATS_NO_WALK 0x80000000u
struct SaStatsParams {
  SaFillParams f;
  int32_t *score;                   /* [n]                                                                             */
  uint32_t *matches, *mismatches;   /* [n]                                                                             */
  uint32_t *err_flag;               /* one word, zeroed by the caller                                                  */
  /* strips only: */
  uint32_t *progress;               /* as SaScoreParams                                                                */
  int32_t *handoff;                 /* as SaSpanParams: per row {max(M, A), B, whether A's, 0} {the two payloads}      */
  const uint64_t *handoff_off;      /* [n], in rows                                                                    */
  uint32_t strips_per_pair;
};
using SaStatsCrossParams = SaCrossParams<SaStatsParams>;
/* recorded as "score_rows" / "score_strips" / "score_cross"; the callers' duties are sa_launch_span_*'s */
hipError_t sa_launch_stats_rows(const SaStatsParams &p, uint32_t max_len_a, hipStream_t stream);
hipError_t sa_launch_stats_strips(const SaStatsParams &p, hipStream_t stream);
hipError_t sa_launch_stats_cross(const SaStatsCrossParams &p, uint32_t max_len_a, hipStream_t stream);
/* ---- SW alignment statistics (seqalign_sw_stats_batch / _cross, sa_sw_stats.hip): the span sweep's SW arithmetic with the
 * span in ONE word and the two counters in the other.  Pair k of a launch: SaSpanParams' five results, and
 * matches[k] / mismatches[k] = the columns of that hit's strings that hold two equal / two different letters (after the
 * scoring's case folding).  Both sequences of every pair have at most SA_SW_STATS_MAX_LEN letters (the caller's duty): a
 * coordinate and a counter are 16 bits each.  Everything else -- row classes, strips, hand-off, progress and strip_best
 * layout -- is SaSpanParams'; a strip_best entry is {score, end_a, end_b, 0} {x | y << 16, matches | mismatches << 16, 0, 0}. */
#define SA_SW_STATS_MAX_LEN SEQALIGN_SW_STATS_MAX_LEN
struct SaSwStatsParams : SaSpanParams {
  uint32_t *matches, *mismatches;   /* [n]                                                                             */
};
using SaSwStatsCrossParams = SaCrossParams<SaSwStatsParams>;
/* recorded as "score_rows" / "score_strips" / "score_cross"; the callers' duties are sa_launch_span_*'s */
hipError_t sa_launch_sw_stats_rows(const SaSwStatsParams &p, uint32_t max_len_a, hipStream_t stream);
hipError_t sa_launch_sw_stats_strips(const SaSwStatsParams &p, hipStream_t stream);
hipError_t sa_launch_sw_stats_cross(const SaSwStatsCrossParams &p, uint32_t max_len_a, hipStream_t stream);
/* ---- SW identity counts (seqalign_sw_counts_batch, sa_sw_counts.hip): the SW statistics sweep with the two counts as two full
 * words and no stop cell, any length.  The span block reused, its four arrays behind the score read as
 *   pos_a = end_a, pos_b = end_b (the best cell, 1-based, as SaScoreParams reports it), len_a = matches, len_b = mismatches;
 * all five are 0 when no cell is above 0.  Everything else -- row classes, strips, hand-off, progress and strip_best layout --
 * is SaSpanParams'; a strip_best entry is {score, end_a, end_b, 0} {matches, mismatches, 0, 0}.  No cross form. */
typedef SaSpanParams SaSwCountsParams;
/* recorded as "score_rows" / "score_strips"; the callers' duties are sa_launch_span_*'s */
hipError_t sa_launch_sw_counts_rows(const SaSwCountsParams &p, uint32_t max_len_a, hipStream_t stream);
hipError_t sa_launch_sw_counts_strips(const SaSwCountsParams &p, hipStream_t stream);
/* ---- SW gap-run counts (seqalign_sw_gaps_batch, sa_sw_gaps.hip): the SW counts sweep with the runs of '-' in the hit's two
 * strings as the two full payload words, any length.  The span block reused, its four arrays behind the score
 * read as
 *   pos_a = end_a, pos_b = end_b (the best cell, 1-based, as SaScoreParams reports it), len_a = gap_runs_a, len_b = gap_runs_b;
 * all five are 0 when no cell is above 0.  Everything else -- row classes, strips, hand-off, progress and strip_best layout --
 * is SaSpanParams'; a strip_best entry is {score, end_a, end_b, 0} {gap_runs_a, gap_runs_b, 0, 0}.  No cross form. */
typedef SaSpanParams SaSwGapsParams;
/* recorded as "score_rows" / "score_strips"; the callers' duties are sa_launch_span_*'s */
hipError_t sa_launch_sw_gaps_rows(const SaSwGapsParams &p, uint32_t max_len_a, hipStream_t stream);
hipError_t sa_launch_sw_gaps_strips(const SaSwGapsParams &p, hipStream_t stream);
/* ---- NW gap-run counts (seqalign_nw_gaps_batch / _cross, sa_nw_gaps.hip): the NW statistics sweep with the runs of '-' in the
 * alignment's two strings as the two payload words, any length.  The statistics block reused, its two arrays
 * behind the score read as
 *   matches = gap_runs_a, mismatches = gap_runs_b; bit 31 of mismatches[k] (SA_STATS_NO_WALK) = the end pick's state has no walk.
 * Everything else -- row classes, strips, hand-off and progress layout -- is SaStatsParams'. */
typedef SaStatsParams SaNwGapsParams;
typedef SaStatsCrossParams SaNwGapsCrossParams;
/* recorded as "score_rows" / "score_strips" / "score_cross"; the callers' duties are sa_launch_stats_*'s */
hipError_t sa_launch_nw_gaps_rows(const SaNwGapsParams &p, uint32_t max_len_a, hipStream_t stream);
hipError_t sa_launch_nw_gaps_strips(const SaNwGapsParams &p, hipStream_t stream);
hipError_t sa_launch_nw_gaps_cross(const SaNwGapsCrossParams &p, uint32_t max_len_a, hipStream_t stream);
/* top-k score search (seqalign_*_score_search, sa_score_select.hip): one workgroup per query row of a tile, after its
 * score_cross launches.  Keeps the k smallest keys (~(score ^ 0x80000000)) << 32 | (t_base + t) of the row's entries with
 * score >= min_score together with the query's running list, and writes them back sorted.  The running list's targets
 * are all below t_base; the caller zeroed list_n before the query range's first target range. */
struct SaScoreSelectParams {
  const int32_t *score;              /* [q * n_t + t] the tile's rows (score_cross_kernel's layout)                       */
  const uint32_t *end_a, *end_b;     /* same layout (SW); NULL: zeros (NW)                                                */
  uint32_t nq, n_t;                  /* rows, and targets per row                                                         */
  uint32_t t_base;                   /* index in the whole target set of the tile's target 0                              */
  uint32_t k;                        /* 1 .. SEQALIGN_SEARCH_MAX_K                                                        */
  uint32_t u_max;                    /* ~(min_score ^ 0x80000000): an entry passes when its key's high word is <= u_max    */
  unsigned long long *list_key;      /* [nq * k] the running lists, sorted, list_n[q] of them valid                       */
  uint32_t *list_ea, *list_eb;       /* [nq * k] their end coordinates                                                    */
  uint32_t *list_n;                  /* [nq]                                                                              */
};
hipError_t sa_launch_score_select(const SaScoreSelectParams &p, hipStream_t stream);
/* alignments of pairs of any size (seqalign_*_align_long, sa_align_long.hip): ONE pair per launch, its descriptors at index 0
 * of f's arrays.  Forward: the score-strips pipeline over the whole pair, which also stores M, A, B of every column at rows
 * R, 2R, .. < len_b (checkpoints).  Block: M, A, B of rows [y0, y1] x columns [0, x] from the checkpoint at y0 (or row 0)
 * into f.M / f.A / f.B at pitch x + 1.  Walk: alignment_reverse_move over the block, one lane, from the state in *walk. */
struct SaLongWalk {
  uint32_t x, y;                /* where the walk stands                                                                */
  int32_t matrix, score;        /* its state                                                                           */
  uint32_t head;                /* the strings are written backwards from out_a / out_b[len_a + len_b]                  */
  uint32_t status;              /* 0 or SEQALIGN_E_UNKNOWN_PAIR / SEQALIGN_E_TRACEBACK                                 */
  uint32_t started, done;       /* the end cell has been read; the walk is over                                        */
  int32_t end_score;
  uint32_t end_x, end_y, pad;
};
struct SaLongParams {
  SaFillParams f;               /* n_pairs = 1; f.status: the lowest cell without a score (forward / block), ~0 = none */
  uint32_t *progress;           /* [strips + 1] zeroed: rows done per strip, then the ticket counter                   */
  uint32_t strips;              /* forward: ceil(len_a / 512) (at least 1); block: ceil(x / 512) (at least 1)          */
  uint32_t R;                   /* rows per block; checkpoints at R, 2R, .. < len_b (R >= len_b: none)                 */
  int32_t *ckpt;                /* checkpoint k at row (k + 1) R: M, A, B of columns 0 .. len_a, 3 (len_a + 1) int32   */
  /* forward */
  int32_t *handoff;             /* strips 0 .. strips - 2: rows 0 .. len_b of {max(M, A), B} of the strip's last column */
  uint32_t *strip_best;         /* [4 * strips] SW: the best cell of strips 0 .. s                                     */
  int32_t *result;              /* [4] score, end_a, end_b (SW: the best cell in hit order), err_flag                  */
  /* block */
  uint32_t y0, y1, x;
  /* walk */
  SaLongWalk *walk;
  char *out_a, *out_b;          /* len_a + len_b bytes each                                                            */
};
#define SA_LONG_STRIP_COLS 512u
hipError_t sa_launch_long_forward(const SaLongParams &p, bool is_sw, hipStream_t stream);
hipError_t sa_launch_long_block(const SaLongParams &p, hipStream_t stream);
hipError_t sa_launch_long_walk(const SaLongParams &p, hipStream_t stream);
/* ---- banded NW (seqalign_nw_*_banded, sa_band.hip): one wave per pair, a frame of 64 x CPL cells that follows the band down
 * the matrix.  Pair k of a launch has the band d_lo[k] <= i - j <= d_lo[k] + width[k] - 1 (width <= SA_BAND_MAX_WIDTH; the
 * caller clamps it to the matrix, include/seqalign_hip.h).  Score form: score[k] = the end cell's max(M, A, B).  Fill form: M, A, B of every band
 * cell, borders included: cell (i, j) at f.mat_off[k] + j (width - 1) + i - d_lo of f.M / f.A / f.B ((len_b + 1) width cells per
 * pair; slots whose column lies outside 0 .. len_a are not written).  Both: f.status[k] = the lowest band cell without a score
 * (~0: none), *err_flag |= 1 when a pair has one.  Walk: one lane per pair over the fill form's cells -- a cell outside the band
 * reads as the floor -- strings written backwards from out_a / out_b + str_off[k] + len_a + len_b, meta4[4k..] = head, length,
 * score, status (0, SEQALIGN_E_UNKNOWN_PAIR, SEQALIGN_E_TRACEBACK). */
#define SA_BAND_MAX_WIDTH 1024u
struct SaBandParams {
  SaFillParams f;
  const int32_t *d_lo;
  const uint32_t *width;
  int32_t *score;
  uint32_t *err_flag;
  const uint64_t *str_off;
  char *out_a, *out_b;
  uint32_t *meta4;
};
/* every pair of the launch has width <= max_width <= SA_BAND_MAX_WIDTH; max_width picks the columns per lane */
hipError_t sa_launch_band_score(const SaBandParams &p, uint32_t max_width, hipStream_t stream);
hipError_t sa_launch_band_fill(const SaBandParams &p, uint32_t max_width, hipStream_t stream);
hipError_t sa_launch_band_walk(const SaBandParams &p, hipStream_t stream);
/* ---- banded SW (seqalign_sw_*_banded, sa_band.hip): the same sweep over the caller's band d_lo[k] <= i - j <= d_lo[k] + width[k]
 * - 1, already clipped to [-len_b, len_a] (1 <= width <= SA_BAND_MAX_WIDTH; a band without an inner cell is legal), every cell
 * outside it and every border cell 0.  Both forms: b.score[k], end_a[k], end_b[k] = the best match_scores cell of the band in
 * hit order, as SaScoreParams reports it; b.f.status / b.err_flag as above.  Fill form: M, A, B of the rows that have inner band
 * cells (sa_band_sw_rows: j0 .. j1), cell (i, j) at b.f.mat_off[k] + (j - j0) width + i - j - d_lo.  Walk: from that best cell
 * until the score is 0, one lane per pair; meta8[8k..] = score, status, pos_a, pos_b, end_a, end_b, length, head. */
struct SaBandSwParams {
  SaBandParams b;               /* b.meta4 unused */
  uint32_t *end_a, *end_b;
  uint32_t *meta8;
};
/* the rows of a banded-SW pair that have inner band cells: *j0 .. *j1 (none: *j1 < *j0) */
static inline void sa_band_sw_rows(uint32_t len_a, uint32_t len_b, int64_t d_lo, int64_t d_hi, int64_t *j0, int64_t *j1) {
  *j0 = d_hi < 0 ? 1 - d_hi : 1;
  *j1 = len_a == 0 ? 0 : ((int64_t)len_a - d_lo < (int64_t)len_b ? (int64_t)len_a - d_lo : (int64_t)len_b);
}
hipError_t sa_launch_band_sw_score(const SaBandSwParams &p, uint32_t max_width, hipStream_t stream);
hipError_t sa_launch_band_sw_fill(const SaBandSwParams &p, uint32_t max_width, hipStream_t stream);
hipError_t sa_launch_band_sw_walk(const SaBandSwParams &p, hipStream_t stream);
/* ---- banded SW hit spans (seqalign_sw_span_banded, sa_band_span.hip): the banded SW score sweep with SaSpanParams' results.
 * Pair k of a launch has the clipped band of SaBandSwParams (1 <= width <= SA_SPAN_BAND_MAX_WIDTH); b.score[k], pos_a[k],
 * pos_b[k], len_a[k], len_b[k] = the fields of the first hit over the banded matrices (all 0 when no band cell is above 0);
 * b.f.status / b.err_flag as above.  b.str_off, b.out_a, b.out_b and b.meta4 are unused. */
#define SA_SPAN_BAND_MAX_WIDTH 512u
struct SaBandSpanParams {
  SaBandParams b;
  uint32_t *pos_a, *pos_b, *len_a, *len_b;
};
/* every pair of the launch has width <= max_width <= SA_SPAN_BAND_MAX_WIDTH; max_width picks the columns per lane */
hipError_t sa_launch_band_span(const SaBandSpanParams &p, uint32_t max_width, hipStream_t stream);
/* ---- banded SW statistics (seqalign_sw_stats_banded, sa_band_stats.hip): the banded span sweep with SaSwStatsParams' payload,
 * the stop cell in one word and matches | mismatches << 16 in the other.  Pair k of a launch has the band of SaBandSpanParams
 * (1 <= width <= SA_SPAN_BAND_MAX_WIDTH) and at most SA_SW_STATS_MAX_LEN letters in either sequence (the caller's duty);
 * b.score[k], pos_a[k], pos_b[k], len_a[k], len_b[k] are sa_launch_band_span's, matches[k] / mismatches[k] the columns of that
 * hit's strings that hold two equal / two different letters (all 0 when no band cell is above 0); b.f.status / b.err_flag as
 * above.  b.str_off, b.out_a, b.out_b and b.meta4 are unused. */
struct SaBandSwStatsParams {
  SaBandParams b;
  uint32_t *pos_a, *pos_b, *len_a, *len_b, *matches, *mismatches;
};
/* recorded as "band_score"; max_width as sa_launch_band_span */
hipError_t sa_launch_band_sw_stats(const SaBandSwStatsParams &p, uint32_t max_width, hipStream_t stream);
/* ---- banded SW identity counts (seqalign_sw_counts_banded, sa_band_counts.hip): the banded span sweep with SaSwCountsParams'
 * payload, matches and mismatches as two full words, any length.  The banded span block reused as SaSwCountsParams reuses the
 * span block: pos_a = end_a, pos_b = end_b, len_a = matches, len_b = mismatches (all 0 when no band cell is above 0). */
typedef SaBandSpanParams SaBandSwCountsParams;
/* recorded as "band_score"; max_width as sa_launch_band_span */
hipError_t sa_launch_band_sw_counts(const SaBandSwCountsParams &p, uint32_t max_width, hipStream_t stream);
/* ---- banded SW gap-run counts (seqalign_sw_gaps_banded, sa_band_gaps.hip): the banded span sweep with SaSwGapsParams' payload,
 * gap_runs_a and gap_runs_b as two full words, any length.  The banded span block reused as SaSwGapsParams reuses the span
 * block: pos_a = end_a, pos_b = end_b, len_a = gap_runs_a, len_b = gap_runs_b (all 0 when no band cell is above 0). */
typedef SaBandSpanParams SaBandSwGapsParams;
/* recorded as "band_score"; max_width as sa_launch_band_span */
hipError_t sa_launch_band_sw_gaps(const SaBandSwGapsParams &p, uint32_t max_width, hipStream_t stream);
/* ---- banded NW statistics (seqalign_nw_stats_banded, sa_band_nw_stats.hip): SaStatsParams' payload through the NW band frame.
 * Pair k of a launch has the band of sa_launch_band_score (d_lo <= 0 <= d_hi, 1 <= width <= SA_SPAN_BAND_MAX_WIDTH) and any
 * length; b.score[k] is sa_launch_band_score's value, matches[k] / mismatches[k] the counts of the alignment inside the band
 * that ends in the end pick's state, bit 31 of mismatches[k] (SA_STATS_NO_WALK) = that state has no walk; b.f.status /
 * b.err_flag as above.  b.str_off, b.out_a, b.out_b and b.meta4 are unused. */
struct SaBandNwStatsParams {
  SaBandParams b;
  uint32_t *matches, *mismatches;
};
/* every pair of the launch has width <= max_width <= SA_SPAN_BAND_MAX_WIDTH; max_width picks the columns per lane */
hipError_t sa_launch_band_nw_stats(const SaBandNwStatsParams &p, uint32_t max_width, hipStream_t stream);
/* ---- banded NW gap-run counts (seqalign_nw_gaps_banded, sa_band_nw_gaps.hip): SaNwGapsParams' payload through the same frame.
 * The banded statistics block reused: matches = gap_runs_a, mismatches = gap_runs_b of the alignment inside the band, the mark
 * where it was. */
typedef SaBandNwStatsParams SaBandNwGapsParams;
hipError_t sa_launch_band_nw_gaps(const SaBandNwGapsParams &p, uint32_t max_width, hipStream_t stream);
/* ---- the wide banded calls (seqalign_*_banded_wide): the same bands, matrices, results and layouts at any width, one wave
 * per (pair, strip of strip_cols columns) in the strips pipeline (sa_band_pipe.hpp).  A launch's block is the narrow launch's
 * record s and the pipeline's words w, the same for every family.  s.b.f.status (NW score and align: s.b alone is used) must hold
 * ~0 per pair before the launch (the strips atomicMin into it).  Pair k has max(1, ceil(len_a / strip_cols)) strips <=
 * strips_per_pair; strip t of it owns progress word slot_off[k] + t (zero before the launch; ~0: all its rows), the family's
 * best entry at slot slot_off[k] + t of strip_best (16-byte aligned; the SW families) and the `width` hand-off entries from
 * entry hand_off[k] + t width of handoff (16-byte aligned).  *ticket (zero before the launch) deals the strips out; front[k]
 * (zero before the launch) counts the publications of pair k's strips; *give_up (zero before the launch) becomes k + 1 for the
 * first pair k of the launch one of whose strips ran out of its wait budget: the results are void then.
 * Every launch: strip_cols 64 | 128 | 256 | 512; items: what the launch record counts (the (pair, strip) waves that sweep a row). */
struct SaBandStripsLayout {
  uint32_t strips_per_pair;
  const uint64_t *slot_off, *hand_off;
  uint32_t *progress, *ticket, *front, *strip_best, *give_up;
  int32_t *handoff;
};
template <class S>
struct SaBandWideParams {
  S s;                          /* first: the offsets of the kernel's arguments behind it are the family's own */
  SaBandStripsLayout w;
};
/* score and align, NW and SW (sa_band_strips.hip): a hand-off entry is the int2 {max(M, A), B} of the strip's last column, a best
 * entry {score, end_a, end_b, 0}.  The walks are sa_launch_band_walk / sa_launch_band_sw_walk over the fill form's cells. */
hipError_t sa_launch_band_strips(const SaBandWideParams<SaBandSwParams> &p, uint32_t strip_cols, bool fill, bool is_sw, uint64_t items, hipStream_t stream);
/* the payload families: sa_launch_band_nw_stats' / sa_launch_band_sw_stats' / sa_launch_band_span's results, recorded as
 * "band_score".  A hand-off entry is SA_BAND_STATS_HANDOFF_BYTES: {max(M, A), B, whether max(M, A) is an admitted A's, 0} {the
 * two payload words of each}; a best entry SA_SPAN_BEST_BYTES: {score, end_a, end_b, 0} {its two payload words, 0, 0}.
 * NW statistics (sa_band_nw_stats_strips.hip): the words are matches and mismatches; there is no best cell, strip_best is unused.
 * SW statistics (sa_band_stats.hip): word 0 the stop cell x | y << 16, word 1 matches | mismatches << 16; both sequences of every
 * pair have at most SA_SW_STATS_MAX_LEN letters.  SW hit spans (sa_band_span.hip): the stop cell's x and y, any length.  SW
 * identity counts (sa_band_counts.hip): matches and mismatches, any length.  SW gap-run counts (sa_band_gaps.hip): gap_runs_a
 * and gap_runs_b, any length.  NW gap-run counts (sa_band_nw_gaps.hip): gap_runs_a and gap_runs_b with the NW mark, no best cell. */
#define SA_BAND_STATS_HANDOFF_BYTES 32u
hipError_t sa_launch_band_sw_counts_strips(const SaBandWideParams<SaBandSwCountsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream);
hipError_t sa_launch_band_sw_gaps_strips(const SaBandWideParams<SaBandSwGapsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream);
hipError_t sa_launch_band_nw_stats_strips(const SaBandWideParams<SaBandNwStatsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream);
hipError_t sa_launch_band_nw_gaps_strips(const SaBandWideParams<SaBandNwGapsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream);
hipError_t sa_launch_band_sw_stats_strips(const SaBandWideParams<SaBandSwStatsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream);
hipError_t sa_launch_band_span_strips(const SaBandWideParams<SaBandSpanParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream);
/* the second launch record (seqalign_ctx_last_call_info_ext: SEQALIGN_KX_*) */
void sa_record_launch_ext(int kind, uint64_t items);
/* long rows (1024..4095 columns), fast-path scorings: one workgroup per pair, shared LDS ring */
bool sa_wgstream_kernel_applicable(const SaFillParams &p, uint32_t max_len_a);
hipError_t sa_launch_fill_wgstream(const SaFillParams &p, uint32_t max_len_a, hipStream_t stream);
bool sa_wgstream_kernel_reports_best(const SaFillParams &p, uint32_t max_len_a, uint32_t max_len_b);
bool sa_wgstream_kernel_emits_candidates(const SaFillParams &p, uint32_t max_len_a);
/* the SW multi-hit path's own fill (sa_fill_dirs.hip): match_scores + one byte of directions per cell into `dirs`
 * (same cell offsets as the matrices), candidates reported as by the stream kernel; plain SW scorings, rows <= 1 024 columns */
bool sa_dirs_fill_applicable(const SaFillParams &p, uint32_t max_len_a, const uint8_t *dirs);
hipError_t sa_launch_fill_dirs(const SaFillParams &p, uint32_t max_len_a, uint8_t *dirs, hipStream_t stream);
/* seqalign_nw_batch's own fill: ONLY the directions (1 B per cell) + per pair the end cell's score (p.best_score) and state
 * (p.best_index); plain NW scorings (no flag), rows <= 1 024 columns */
bool sa_nw_dirs_fill_applicable(const SaFillParams &p, uint32_t max_len_a, const uint8_t *dirs);
hipError_t sa_launch_fill_nw_dirs(const SaFillParams &p, uint32_t max_len_a, uint8_t *dirs, hipStream_t stream);
/* the same fills with two pairs per wave in packed int16 (sa_fill_dirs_x2.hip): uniform batches, match / mismatch scorings,
 * scores inside int16 */
bool sa_x2_scores_fit(const SaFillParams &p, uint32_t max_len_a, uint32_t max_len_b);
bool sa_nw_dirs_x2_applicable(const SaFillParams &p, uint32_t max_len_a, uint32_t max_len_b, const uint8_t *dirs);
hipError_t sa_launch_fill_nw_dirs_x2(const SaFillParams &p, uint32_t max_len_a, uint8_t *dirs, hipStream_t stream);
hipError_t sa_launch_fill_nw_dirs_mixed(const SaFillParams &p, uint32_t max_len_a, uint8_t *dirs, uint32_t n_modal, uint32_t n_rest,
                                        hipStream_t stream);
bool sa_sw_best_x2_applicable(const SaFillParams &p, uint32_t max_len_a, uint32_t max_len_b, const uint8_t *dirs);
hipError_t sa_launch_fill_sw_best_x2(const SaFillParams &p, uint32_t max_len_a, uint8_t *dirs, hipStream_t stream);
bool sa_dirs_x2_applicable(const SaFillParams &p, uint32_t max_len_a, uint32_t max_len_b, const uint8_t *dirs);
hipError_t sa_launch_fill_dirs_x2(const SaFillParams &p, uint32_t max_len_a, uint8_t *dirs, hipStream_t stream);
hipError_t sa_launch_sw_reduce(const SaReduceParams &p, hipStream_t stream);
/* candidates' count and box from match_scores already in HBM (fills that cannot report them themselves): one
 * pass over M */
hipError_t sa_launch_sw_box(const SaReduceParams &p, const SaCandBox &c, uint32_t max_len_b, hipStream_t stream);
/* SW multi-hit enumeration (sa_sw_sweep.hip): every hit of every pair in one reverse sweep, then one traceback
 * per wanted hit (sa_launch_nw_traceback with SaTraceParams::hit_keys), then the strings packed back to back (walk
 * w's len[w] chars at head[w] of its slot to dst_off[w]) */
hipError_t sa_launch_sw_sweep(const SaSweepParams &p, hipStream_t stream);
hipError_t sa_launch_gather_hits(const char *src_a, const char *src_b, const uint64_t *walker_str, const uint32_t *head,
                                 const uint32_t *len, const uint64_t *dst_off, char *dst_a, char *dst_b, uint32_t n_walkers,
                                 hipStream_t stream);
hipError_t sa_launch_nw_traceback(const SaTraceParams &p, hipStream_t stream);
/* the three matrix arenas, placed and checked (sa_placement.hip) */
#define SA_ARENA_MAX_TRIES 96
struct SaArenaInfo {   /* = seqalign_arena_info_t (include/seqalign_hip.h) */
  float quality, target;
  int32_t vmm;
  uint32_t chunk_mib;
  float depth_gib, scanned_gib, depth_a_gib;
  uint32_t tries, second_walk_from;
  float try_quality[SA_ARENA_MAX_TRIES], try_depth_gib[SA_ARENA_MAX_TRIES];
  float kept_gib;
  float seconds;
};
struct SaPlacementOpts {
  size_t scan_bytes;     /* device memory the walk may hold transiently besides the arenas; 0 = allocate plainly */
  float quality_stop;    /* probe ratio that ends the walk */
  float free_fraction;   /* ... and never more than this share of the memory free at its start (0: the default, 0.6) */
  size_t keep_bytes;     /* how much of the walk's unused chunks stays with the process (the chunk pool) instead of going back */
};
/* the per-device chunk pool (sa_placement.hip): large scratch buffers mapped from chunks a walk left behind */
void *sa_pool_alloc(int device, size_t bytes);   /* NULL: the pool cannot serve it (allocate plainly) */
bool sa_pool_free(void *ptr);                    /* false: not a pool buffer (hipFree it) */
size_t sa_pool_bytes(int device);
void sa_pool_trim(int device, size_t keep_bytes);
void sa_pool_ref(int device);
void sa_pool_unref(int device);
struct SaArenaSet;
hipError_t sa_arenas_create(int device, size_t bytes, hipStream_t stream, const SaPlacementOpts &opt, SaArenaSet **out);
void sa_arenas_destroy(SaArenaSet *s);
SaArenaSet *sa_arenas_take(void *base0);   /* removes the set from the registry (seqalign_arenas_free); NULL if unknown */
const SaArenaInfo *sa_arenas_info(const SaArenaSet *s);
bool sa_arenas_copy_info(void *base0, SaArenaInfo *out);   /* false: not arenas of sa_arenas_create */
void *const *sa_arenas_base(const SaArenaSet *s);
size_t sa_arenas_bytes(const SaArenaSet *s);
/* DPP self-test: out[l] = value shifted in from lane l-1 (lane 0 gets `fill`) */
hipError_t sa_launch_dpp_probe(int32_t *out64, int32_t fill, hipStream_t stream);

#endif
