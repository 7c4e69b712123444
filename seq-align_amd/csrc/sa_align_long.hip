// sa_align_long.hip -- alignments of pairs of any size (seqalign_nw_align_long / seqalign_sw_align_long, sa_batch_long.hip):
// the three matrices of a pair are never held whole.  One pair at a time:
//
//   long_forward  score_strips_kernel (sa_score.hip; the pipeline: sa_strips.hpp) over the whole pair, the ticket being the
//                 strip -- and at rows R, 2R, .. < len_b every strip also stores M, A, B of its columns: the checkpoints,
//                 12 B x (len_a + 1) each.  Yields the NW score, or the SW best cell in hit order.
//   long_block    M, A, B of rows [y0, y1] x columns [0, x] -- the rows from the checkpoint at y0 (or the border row 0) down to
//                 where the walk stands, the columns left of it -- into a block buffer at pitch x + 1.  The same pipeline
//                 as sa_fill_strips.hip, strip s reading strip s - 1's last column back from the block; RowSweep starts from
//                 the stored row instead of row 0 (start_from_row below).  Every rule that depends on where a cell lies (the
//                 border, the GENERAL path's last row / column, no_gaps_in_*) sees the GLOBAL row index and the pair's true
//                 len_a / len_b: a block's values are the full matrix's, bit for bit.
//   long_walk     alignment_reverse_move's decision order (reverse_move_t, sa_trace_common.hpp) over the block, one lane,
//                 until the next predecessor would lie above y0; the state (x, y, matrix, score, output position) stays in
//                 device memory for the next block.  The strings are written backwards, as traceback_kernel writes them.
// SW needs no second forward pass: the rectangle [0 .. end_a] x [0 .. end_b] holds the full matrix's values, and its
// checkpoints are prefixes of the stored rows.
#include "sa_strips.hpp"
#include "sa_trace_common.hpp"

namespace sa {

constexpr int kLongCPL = 8;                          // 512 columns per strip, as sa_fill_strips.hip / sa_score.hip
constexpr uint32_t kLongCols = kWave * kLongCPL;
static_assert(kLongCols == SA_LONG_STRIP_COLS, "strip width");

// my CPL columns of one row into M / A / B at dst (columns past ncol are not mine to write)
template <int CPL>
__device__ __forceinline__ void long_store_row(int32_t *M, int32_t *A, int32_t *B, uint64_t at, int ncol, const int (&mv)[CPL],
                                               const int (&av)[CPL], const int (&bv)[CPL]) {
  if (ncol == CPL) {
    store_run<CPL>(M + at, mv); store_run<CPL>(A + at, av); store_run<CPL>(B + at, bv);
  } else if (ncol > 0) {
    store_partial<CPL>(M + at, mv, ncol); store_partial<CPL>(A + at, av, ncol); store_partial<CPL>(B + at, bv, ncol);
  }
}

// ---------------------------------------------------------------------------------------------------------- forward ---
template <int SUBST, bool GENERAL, bool SW>
__global__ void __launch_bounds__(kWave) long_forward_kernel(const SaLongParams lp) {
  constexpr int CPL = kLongCPL;
  const SaFillParams &p = lp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x;
  const uint32_t strip = strip_ticket(lp.progress + lp.strips);   // (the counter sits behind the progress words)
  const uint32_t la = p.len_a[0], lb = p.len_b[0];
  const uint32_t i0 = strip * kLongCols;
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[0];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[0];
  const uint32_t W = la + 1;
  uint32_t *done = lp.progress;
  const uint64_t rows = (uint64_t)lb + 1;
  int32_t *hand_out = lp.handoff + 2 * ((uint64_t)strip * rows);
  const int32_t *hand_in = lp.handoff + 2 * ((uint64_t)(strip ? strip - 1 : 0) * rows);
  const uint32_t R = lp.R;

  const SweepConsts k(p, table);
  const Border bd{p.floor, p.gap_open, p.ext, SW, (p.flags & SA_F_NO_START_GAP) != 0};

  const uint32_t cols = (i0 < la) ? min(kLongCols, la - i0) : 0;
  const bool last_strip = i0 + kLongCols >= la;
  const uint32_t col0 = i0 + lane * CPL;
  const int ncol = max(0, min(CPL, (int)cols - lane * CPL));
  RowSweep<CPL, SUBST, GENERAL> sw;
  sw.start_strip(p, k, bd, sa_, la, i0, col0, lane);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  int best_s[SW ? CPL : 1];   // BestCells, open-coded: with the struct this kernel's SW forms ran 1 % slower (profiles/r11)
  uint32_t best_r[SW ? CPL : 1];
#pragma unroll
  for (int c = 0; c < (SW ? CPL : 1); ++c) { best_s[c] = 0; best_r[c] = 0; }

  StripHandoff h;
  uint32_t to_ck = R;             // rows until the next checkpoint row
  uint64_t ck_at = (uint64_t)col0 + 1;
  for (uint32_t j = 1; j <= lb; ++j) {
    const int q = (j - 1) & (kWave - 1);
    if (q == 0) {
      if (strip > 0) strip_wait(done + strip - 1, min(j + kWave - 1, lb));
      h.load(p, k, bd, sb_, lb, strip, hand_in, j + lane);
    }
    int mv[CPL], av[CPL], bv[CPL];
    sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(h.code, q), read_lane(h.fz, q), read_lane(h.fb, q), mv, av, bv);
    if constexpr (SW) {
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const bool up = mv[c] > best_s[c];   // strict: the first (lowest) row keeps a tie
        best_s[c] = up ? mv[c] : best_s[c];
        best_r[c] = up ? j : best_r[c];
      }
    }
    if (--to_ck == 0) {   // a checkpoint row (R >= len_b: never reached before the last row, which is not one)
      to_ck = R;
      if (j < lb) {
        long_store_row<CPL>(lp.ckpt, lp.ckpt + W, lp.ckpt + 2ull * W, ck_at, ncol, mv, av, bv);
        ck_at += 3ull * W;
      }
    }
    if (!last_strip) h.keep<CPL>(mv, av, bv, hand_out, done + strip, lane, q, j, lb);
  }

  const unsigned long long err = sw.reduce_err();
  if (lane == 0 && err != ~0ull) {
    atomicMin(reinterpret_cast<unsigned long long *>(p.status), err);
    atomicOr(reinterpret_cast<uint32_t *>(lp.result + 3), 1u);
  }
  if constexpr (SW) {
    int b = 0;
    unsigned long long kb = ~0ull;
#pragma unroll
    for (int c = 0; c < CPL; ++c)   // c ascending, strict >: the lowest column wins a tie
      if (c < ncol && best_s[c] > b) { b = best_s[c]; kb = ((unsigned long long)(col0 + c + 1) << 32) | best_r[c]; }
    int score = wave_max_i32(b);
    unsigned long long key = wave_min_u64(b == score && score > 0 ? kb : ~0ull);
    if (strip > 0 && lb > 0) merge_left_best(lp.strip_best + 4ull * (strip - 1), score, key);
    const uint32_t ea = score > 0 ? (uint32_t)(key >> 32) : 0u, eb = score > 0 ? (uint32_t)key : 0u;
    if (lane == 0) {
      if (last_strip) {
        lp.result[0] = score; lp.result[1] = (int32_t)ea; lp.result[2] = (int32_t)eb;
      } else {
        *reinterpret_cast<uint4 *>(lp.strip_best + 4ull * strip) = make_uint4((uint32_t)score, ea, eb, 0u);
      }
    }
  } else if (last_strip) {
    if (la == 0) {   // cell (0, len_b) of the border column
      if (lane == 0) lp.result[0] = lb == 0 ? 0 : max(k.floor_, bd.edge_gap(lb));
    } else {
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        if (col0 + c + 1 == la) lp.result[0] = sw.X[c];   // max(M, A, B) of (len_a, len_b)
    }
  }
  if (!last_strip && lb > 0) strip_publish(done + strip, lb);   // the last rows (and the best cell so far)
}

// ------------------------------------------------------------------------------------------------------------ block ---
// RowSweep's state as if it had just produced row y0 > 0: X = max3(M, A, B), Y = max(M, B), Ap = A of my columns from the
// checkpoint row, boundX = max3 of the cell left of the strip (column 0 of row y0: the border)
template <int CPL, int SUBST, bool GENERAL>
__device__ __forceinline__ void start_from_row(RowSweep<CPL, SUBST, GENERAL> &sw, const SweepConsts &k, const Border &bd,
                                               const int32_t *__restrict__ ck, uint32_t W, uint32_t x, uint32_t i0,
                                               uint32_t col0, uint32_t y0) {
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const uint32_t idx = col0 + c + 1;
    int m = k.floor_, a = k.floor_, b = k.floor_;
    if (idx <= x) { m = ck[idx]; a = ck[W + idx]; b = ck[2ull * W + idx]; }
    sw.X[c] = max3i(m, a, b);
    if constexpr (GENERAL) sw.Y[c] = max(m, b);
    sw.Ap[c] = a;
  }
  sw.boundX = (i0 == 0) ? max(k.floor_, bd.edge_gap(y0)) : max3i(ck[i0], ck[W + i0], ck[2ull * W + i0]);
}

template <int SUBST, bool GENERAL>
__global__ void __launch_bounds__(kWave) long_block_kernel(const SaLongParams lp) {
  constexpr int CPL = kLongCPL;
  const SaFillParams &p = lp.f;
  extern __shared__ __attribute__((aligned(16))) int32_t lds_table[];
  const int32_t *table = stage_table<SUBST>(p, lds_table);

  const int lane = threadIdx.x;
  const uint32_t strip = strip_ticket(lp.progress + lp.strips);   // (the counter sits behind the progress words)
  const uint32_t la = p.len_a[0], lb = p.len_b[0];
  const uint32_t x = lp.x, y0 = lp.y0, y1 = lp.y1;
  const uint32_t i0 = strip * kLongCols;
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[0];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[0];
  const uint32_t W = la + 1;     // the pair's pitch (checkpoints, error index)
  const uint64_t Wb = (uint64_t)x + 1;   // the block's
  int32_t *__restrict__ Mb = p.M;
  int32_t *__restrict__ Ab = p.A;
  int32_t *__restrict__ Bb = p.B;
  uint32_t *done = lp.progress;
  const int32_t *ck = y0 ? lp.ckpt + (uint64_t)(y0 / lp.R - 1) * 3ull * W : nullptr;

  const SweepConsts k(p, table);
  const Border bd{p.floor, p.gap_open, p.ext, (p.flags & SA_F_IS_SW) != 0, (p.flags & SA_F_NO_START_GAP) != 0};

  // ---- row y0 over my columns, column 0 by strip 0 (reference alignment.c:46-81 at y0 = 0)
  const uint32_t cols = (i0 < x) ? min(kLongCols, x - i0) : 0;
  for (uint32_t i = i0 + 1 + lane; i <= i0 + cols; i += kWave) {
    if (y0 == 0) { Mb[i] = k.floor_; Ab[i] = k.floor_; Bb[i] = bd.edge_gap(i); }
    else { Mb[i] = ck[i]; Ab[i] = ck[W + i]; Bb[i] = ck[2ull * W + i]; }
  }
  if (strip == 0) {
    if (lane == 0) {
      Mb[0] = y0 ? k.floor_ : 0; Ab[0] = y0 ? bd.edge_gap(y0) : 0; Bb[0] = y0 ? k.floor_ : 0;
    }
    for (uint32_t j = y0 + 1 + lane; j <= y1; j += kWave) {
      const uint64_t c = (uint64_t)(j - y0) * Wb;
      Mb[c] = k.floor_;
      Ab[c] = bd.edge_gap(j);
      Bb[c] = k.floor_;
    }
  }

  unsigned long long err = ~0ull;
  if (cols) {
    RowSweep<CPL, SUBST, GENERAL> sw;
    const uint32_t col0 = i0 + lane * CPL;
    const int ncol = max(0, min(CPL, (int)cols - lane * CPL));
    sw.start_strip(p, k, bd, sa_, la, i0, col0, lane);
    __builtin_amdgcn_s_waitcnt(kWaitVm0);   // seq_a codes landed (see RowFeed::load)
    if (y0) start_from_row(sw, k, bd, ck, W, x, i0, col0, y0);
    const bool last_strip = i0 + kLongCols >= x;

    int code = 0, fz = 0, fb = 0;
    uint64_t off = Wb + col0 + 1;            // (block row 1, my first column)
    for (uint32_t j = y0 + 1; j <= y1; ++j, off += Wb) {
      const uint32_t lr = j - y0;            // the block's row
      const int q = (lr - 1) & (kWave - 1);
      if (q == 0) {
        if (strip > 0) strip_wait(done + strip - 1, min(lr + kWave - 1, y1 - y0) + 1);
        const uint32_t r = j + lane;
        if (r <= y1) {
          code = p.code[sb_[r - 1]];
          if (strip == 0) {   // border column (reference alignment.c:72-80)
            fz = max(k.floor_, bd.edge_gap(r));
            fb = k.floor_;
          } else {            // the last column of the strip to my left
            const uint64_t c = (uint64_t)(r - y0) * Wb + i0;
            fz = max(Mb[c], Ab[c]);
            fb = Bb[c];
          }
        }
        __builtin_amdgcn_s_waitcnt(kWaitVm0);
      }
      int mv[CPL], av[CPL], bv[CPL];
      sw.row(k, j, lb, la, W, lane, col0, ncol, read_lane(code, q), read_lane(fz, q), read_lane(fb, q), mv, av, bv);
      long_store_row<CPL>(Mb, Ab, Bb, off, ncol, mv, av, bv);
      if (!last_strip && (q == kWave - 1 || j == y1)) strip_publish(done + strip, lr + 1);   // rows <= lr are written
    }
    err = sw.reduce_err();
  }
  if (lane == 0 && err != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(p.status), err);
}

// ------------------------------------------------------------------------------------------------------------- walk ---
// reverse_move_t's view of a block: global (x, y) -> the block's cell (x, y - y0)
struct BlockAccess {
  const uint8_t *seq_a, *seq_b;
  const uint16_t *code;
  const int32_t *M, *A, *B;
  uint32_t y0;
  uint64_t Wb;
  __device__ __forceinline__ int code_a(uint32_t i) const { return code[seq_a[i]]; }
  __device__ __forceinline__ int code_b(uint32_t j) const { return code[seq_b[j]]; }
  __device__ __forceinline__ void cell(uint32_t x, uint32_t y, int &m, int &a, int &b) const {
    const uint64_t at = (uint64_t)(y - y0) * Wb + x;
    m = M[at]; a = A[at]; b = B[at];
  }
};

__global__ void __launch_bounds__(kWave) long_walk_kernel(const SaLongParams lp) {
  if (threadIdx.x != 0) return;
  const SaFillParams &p = lp.f;
  SaLongWalk *st = lp.walk;
  if (st->done) return;
  const uint32_t la = p.len_a[0], lb = p.len_b[0];
  const uint8_t *__restrict__ sa_ = p.arena + p.off_a[0];
  const uint8_t *__restrict__ sb_ = p.arena + p.off_b[0];
  const bool is_sw = (p.flags & SA_F_IS_SW) != 0;
  const uint32_t y0 = lp.y0;
  const BlockAccess acc{sa_, sb_, p.code, p.M, p.A, p.B, y0, (uint64_t)lp.x + 1};
  const TraceConsts k{p.code, p.table, (int)p.K, p.open1, p.ext, p.gen_eq, p.gen_ne,
                      (p.flags & SA_F_NO_START_GAP) != 0, (p.flags & SA_F_NO_END_GAP) != 0,
                      (p.flags & SA_F_NO_GAPS_A) != 0, (p.flags & SA_F_NO_GAPS_B) != 0};
  char *oa = lp.out_a, *ob = lp.out_b;

  uint32_t x = st->x, y = st->y, head = st->head, err = 0;
  int matrix = st->matrix, score = st->score;
  if (!st->started) {
    int m, a, b;
    acc.cell(x, y, m, a, b);
    matrix = MAT_MATCH;
    score = m;
    if (!is_sw) {   // end cell: ties resolve GAP_A > GAP_B > MATCH (needleman_wunsch.c:53-66)
      if (b >= score) { matrix = MAT_GAP_B; score = b; }
      if (a >= score) { matrix = MAT_GAP_A; score = a; }
    }
    st->started = 1;
    st->end_score = score; st->end_x = x; st->end_y = y;
  }

  bool handoff = false;
  while (is_sw ? (score > 0) : (x > 0 && y > 0)) {
    if (y == y0 && y0 > 0 && matrix != MAT_GAP_B) { handoff = true; break; }   // the predecessor lies in the next block
    // (a state that cannot move -- never reached on the reference's matrices: SW borders are 0 -- ends the walk, not the lane)
    if (head == 0 || (matrix != MAT_GAP_B && y == 0) || (matrix != MAT_GAP_A && x == 0)) { err = 7; break; }
    --head;
    oa[head] = (matrix == MAT_GAP_A) ? '-' : (char)sa_[x - 1];
    ob[head] = (matrix == MAT_GAP_B) ? '-' : (char)sb_[y - 1];
    if ((err = reverse_move_t(acc, k, la, lb, x, y, matrix, score))) break;
  }
  if (!handoff && !err && !is_sw) {
    for (; y > 0; --y) { --head; oa[head] = '-'; ob[head] = (char)sb_[y - 1]; }   // needleman_wunsch.c:117-123
    for (; x > 0; --x) { --head; oa[head] = (char)sa_[x - 1]; ob[head] = '-'; }   // :126-132
  }
  st->x = x; st->y = y; st->matrix = matrix; st->score = score; st->head = head;
  st->status = err;
  st->done = handoff ? 0u : 1u;
}

template <bool SW>
static hipError_t launch_forward(const SaLongParams &p, hipStream_t stream) {
  launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((long_forward_kernel<subst(), general(), SW>), dim3(p.strips), dim3(kWave), table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

}  // namespace sa

hipError_t sa_launch_long_forward(const SaLongParams &p, bool is_sw, hipStream_t stream) {
  if (p.strips == 0 || p.R == 0) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_LONG_FORWARD, 1);
  return is_sw ? sa::launch_forward<true>(p, stream) : sa::launch_forward<false>(p, stream);
}

hipError_t sa_launch_long_block(const SaLongParams &p, hipStream_t stream) {
  using namespace sa;
  if (p.strips == 0 || p.R == 0 || p.y1 < p.y0 || (p.y0 && p.y0 % p.R)) return hipErrorInvalidValue;
  sa_record_launch(SEQALIGN_K_LONG_BLOCK, 1);
  launch_by_scoring(p.f, [&](auto subst, auto general, uint32_t table_ints) {
    hipLaunchKernelGGL((long_block_kernel<subst(), general()>), dim3(p.strips), dim3(kWave), table_ints * sizeof(int32_t), stream, p);
  });
  return hipGetLastError();
}

hipError_t sa_launch_long_walk(const SaLongParams &p, hipStream_t stream) {
  sa_record_launch(SEQALIGN_K_LONG_WALK, 1);
  hipLaunchKernelGGL(sa::long_walk_kernel, dim3(1), dim3(sa::kWave), 0, stream, p);
  return hipGetLastError();
}
