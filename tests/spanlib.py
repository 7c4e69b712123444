"""Helpers of the SW hit-span tests (seqalign_sw_span_batch).  Not a test module.

want_spans          what the call must return, from the oracle's first hit (orclib.oracle_sw, min_score = 1, max_hits = 1);
propagate           the DEFINITION the kernel rests on, in pure Python over the oracle's matrices: the span of (cell, state) is
                    the cell itself where the value is <= 0 or the cell is on the border, else the span of the predecessor
                    alignment_reverse_move picks (priority selectable);
gap_b_sources       along a row, the source of every gap_b cell by the walker's sequential rule and by the ordered-key rule;
kernel_model        the kernel's own shape on the CPU: two merged spans per column across rows, the running maximum along a
                    row with the kernel's one-bit tie rule, strips that hand on {max(M, A), B, whether A, two spans} -- spans only, values from the oracle;
walk_span           the first hit by walking back from the best cell with a selectable priority;
tie_sensitive       how many pairs of a batch change their span when the priority is reversed to M > B > A;
walk_both           one pair's two walks (WALKER, REVERSED) for wide pairs: the oracle's matrices as they come, the best cell
                    found by numpy;
tie_pairs           the tie-dense pairs of one width class (tests/test_gpu_sw_span_dense.py);
flag_pairs          four pairs of one width for the flags that change SpanSweep::row;
walk_seams          one pair's walk, and the walk with the tie order lost on the steps that cross a strip seam only;
seam_pairs          pairs whose hit crosses a seam out of a cell where gap_a and gap_b tie.
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np

import orclib as O

MATCH, GAP_A, GAP_B = O.MATCH, O.GAP_A, O.GAP_B
WALKER = (GAP_A, GAP_B, MATCH)       # alignment_reverse_move's order (alignment.c:311-327)
REVERSED = (MATCH, GAP_B, GAP_A)


class NoPredecessor(Exception):
    """A positive cell none of whose predecessors satisfies the walker's equality (SEQALIGN_E_TRACEBACK)."""


def want_spans(osc, batch):
    """[(score, pos_a, pos_b, len_a, len_b)] per pair: the oracle's first hit, zeros when there is none."""
    out = []
    for p in range(batch.n_pairs):
        rc, hits = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), 1, 1)
        assert rc == 0, (p, rc)
        h = hits[0] if hits else None
        out.append((h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) if h else (0, 0, 0, 0, 0))
    return out


def got_spans(res):
    """sw_span's five arrays as the list want_spans returns."""
    return [tuple(int(x[p]) for x in res) for p in range(len(res[0]))]


class _Lookup:
    """scoring_lookup of the oracle, one call per distinct character pair."""

    def __init__(self, osc):
        self.osc, self.memo, self.lib = osc, {}, O.oracle()

    def __call__(self, ca: int, cb: int) -> int:
        k = (ca, cb)
        if k not in self.memo:
            s, m = C.c_int(0), C.c_int(0)
            rc = self.lib.orc_scoring_lookup(C.byref(self.osc), C.c_char(bytes([ca])), C.c_char(bytes([cb])), C.byref(s), C.byref(m))
            assert rc == 0, (ca, cb)
            self.memo[k] = s.value
        return self.memo[k]


def _matrices(osc, a, b):
    rc, M, A, B = O.oracle_fill(osc, a, b, 1)
    assert rc == 0
    return M.tolist(), A.tolist(), B.tolist()


def best_cell(M, la, lb):
    """The first hit's end cell: score descending, column ascending, row ascending (smith_waterman.c:71-86)."""
    W = la + 1
    best, at = 0, None
    for x in range(1, W):
        for y in range(1, lb + 1):
            if M[y * W + x] > best:
                best, at = M[y * W + x], (x, y)
    return best, at


def propagate(osc, a: bytes, b: bytes, priority=WALKER, mats=None):
    """Forward propagation of the definition.  Returns (span, M, A, B): span[state][y * W + x] = (x0, y0)."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = mats or _matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    look = _Lookup(osc)
    span = {st: [None] * (W * (lb + 1)) for st in (MATCH, GAP_A, GAP_B)}
    for y in range(lb + 1):
        for x in range(W):
            at = y * W + x
            for st in (MATCH, GAP_A, GAP_B):
                v = vals[st][at]
                if v <= 0 or x == 0 or y == 0:
                    span[st][at] = (x, y)
                    continue
                a_open, a_ext, b_open, b_ext = open1, ext, open1, ext      # alignment.c:261-272
                if osc.no_end_gap_penalty:
                    if x == la:
                        a_open = a_ext = 0
                    if y == lb:
                        b_open = b_ext = 0
                if st == MATCH:
                    s = look(a[x - 1], b[y - 1])
                    via, nx, ny = {MATCH: s, GAP_A: s, GAP_B: s}, x - 1, y - 1
                elif st == GAP_A:
                    via, nx, ny = {MATCH: a_open, GAP_A: a_ext, GAP_B: a_open}, x, y - 1
                else:
                    via, nx, ny = {MATCH: b_open, GAP_A: b_open, GAP_B: b_ext}, x - 1, y
                pat = ny * W + nx
                ok = {GAP_A: (not osc.no_gaps_in_a) or nx == 0 or nx == la,
                      GAP_B: (not osc.no_gaps_in_b) or ny == 0 or ny == lb, MATCH: True}
                for s2 in priority:
                    if ok[s2] and vals[s2][pat] + via[s2] == v:
                        span[st][at] = span[s2][pat]
                        break
                else:
                    raise NoPredecessor((x, y, st))
    return span, M, A, B


def _fields(best, at, start):
    if best <= 0:
        return (0, 0, 0, 0, 0)
    return (best, start[0], start[1], at[0] - start[0], at[1] - start[1])


def span_by_propagation(osc, a: bytes, b: bytes, priority=WALKER, mats=None):
    """(score, pos_a, pos_b, len_a, len_b) of the first hit from the forward propagation."""
    span, M, _, _ = propagate(osc, a, b, priority, mats)
    best, at = best_cell(M, len(a), len(b))
    return _fields(best, at, span[MATCH][at[1] * (len(a) + 1) + at[0]] if at else None)


def walk_span(osc, a: bytes, b: bytes, priority=WALKER, mats=None, best=None, seam_priority=None, seam: int = 512, seam_steps=(MATCH, GAP_B)):
    """(score, pos_a, pos_b, len_a, len_b) of the first hit by WALKING back from the best cell with the given priority: what
    the propagation gives for that priority (test_sw_span_argument_cpu.py), at the cost of one path instead of all cells.
    best: best_cell's result where the caller has it already (walk_both).
    seam_priority: another priority for the steps that cross a strip seam of sa_span.hip -- from column k seam + 1 to column
    k seam, in one of the states seam_steps (MATCH: the diagonal step, whose predecessor the right strip takes from the left
    strip's hand-off through `zwins`; GAP_B: the horizontal step, through the opening's kind and the carried chain)."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = mats or _matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    look = _Lookup(osc)
    best, at = best or best_cell(M, la, lb)
    if best <= 0:
        return (0, 0, 0, 0, 0)
    (x, y), st, v = at, MATCH, best
    while v > 0 and x > 0 and y > 0:
        a_open, a_ext, b_open, b_ext = open1, ext, open1, ext
        if osc.no_end_gap_penalty:
            if x == la:
                a_open = a_ext = 0
            if y == lb:
                b_open = b_ext = 0
        if st == MATCH:
            s = look(a[x - 1], b[y - 1])
            via, x, y = {MATCH: s, GAP_A: s, GAP_B: s}, x - 1, y - 1
        elif st == GAP_A:
            via, y = {MATCH: a_open, GAP_A: a_ext, GAP_B: a_open}, y - 1
        else:
            via, x = {MATCH: b_open, GAP_A: b_open, GAP_B: b_ext}, x - 1
        pat = y * W + x
        ok = {GAP_A: (not osc.no_gaps_in_a) or x == 0 or x == la, GAP_B: (not osc.no_gaps_in_b) or y == 0 or y == lb, MATCH: True}
        across = seam_priority is not None and st in seam_steps and st != GAP_A and x > 0 and x % seam == 0
        for s2 in (seam_priority if across else priority):
            if ok[s2] and vals[s2][pat] + via[s2] == v:
                st, v = s2, vals[s2][pat]
                break
        else:
            raise NoPredecessor((x, y, st))
    return _fields(best, at, (x, y))


def tie_sensitive(osc, batch) -> int:
    """Pairs whose span changes when the predecessor priority is reversed to M > B > A."""
    n = 0
    for p in range(batch.n_pairs):
        a, b = batch.seq_a(p), batch.seq_b(p)
        mats = _matrices(osc, a, b)
        n += walk_span(osc, a, b, WALKER, mats) != walk_span(osc, a, b, REVERSED, mats)
    return n


# the ordered key of a candidate of the gap_b chain that enters at column k (sa_span.hip's header)
def key_m(k): return -k - 2
def key_a(k): return 2 * k
def key_floor(k): return 2 * k + 1 if k else -1      # column 0 is the border: what comes in from the left of everything


def gap_b_sources(osc, a: bytes, b: bytes):
    """For a scoring without flags: [(x, y, sequential, keyed)] for every gap_b cell above 0 -- its source ('A' | 'M' | 'F',
    k) by the walker going left step by step, and by the maximum of (value, key) over all candidates."""
    assert not (osc.no_end_gap_penalty or osc.no_gaps_in_a or osc.no_gaps_in_b)
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = _matrices(osc, a, b)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    out = []
    for y in range(1, lb + 1):
        r = y * W
        for g in range(1, W):
            v = B[r + g]
            if v <= 0:
                continue
            j, cur = g, v
            while True:                       # alignment_reverse_move in state GAP_B, until it leaves the chain
                if A[r + j - 1] + open1 == cur:
                    seq = ("A", j)
                    break
                if B[r + j - 1] + ext == cur:
                    cur, j = B[r + j - 1], j - 1
                    if cur == 0:
                        seq = ("F", j)
                        break
                    continue
                assert M[r + j - 1] + open1 == cur, (g, y)
                seq = ("M", j)
                break
            cands = [((g - 0) * ext, key_floor(0), ("F", 0))]
            for k in range(1, g + 1):
                run = (g - k) * ext
                if A[r + k - 1] >= M[r + k - 1]:          # max(M, A) is A's on a tie: the walker asks A first
                    cands.append((A[r + k - 1] + open1 + run, key_a(k), ("A", k)))
                else:
                    cands.append((M[r + k - 1] + open1 + run, key_m(k), ("M", k)))
                cands.append((run, key_floor(k), ("F", k)))
            top = max(cands, key=lambda c: (c[0], c[1]))
            assert top[0] == v, (g, y, top, v)
            out.append((g, y, seq, top[2]))
    return out


def kernel_model(osc, a: bytes, b: bytes, strip_cols: int = 1 << 30):
    """(score, pos_a, pos_b, len_a, len_b) the way the kernel finds it (values from the oracle's matrices, spans carried)."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = _matrices(osc, a, b)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, no_gaps_b = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_b)
    D = [(x, 0) for x in range(W)]          # row 0
    V = [(x, 0) for x in range(W)]
    best, best_at, best_span = 0, None, None
    col_best = [0] * W
    col_info = [None] * W
    for y in range(1, lb + 1):
        r = y * W
        free_row, forced = no_end and y == lb, no_gaps_b and y != lb
        nD, nV = [(0, y)] + [None] * la, [(0, y)] + [None] * la
        feed = dict(z=0, b=0, from_a=False, zs=(0, y), bs=(0, y))      # the border column
        for i0 in range(0, max(la, 1), strip_cols):
            hi = min(la, i0 + strip_cols)
            # the diagonal feed of the boundary cell on the PREVIOUS row was derived from that row's hand-off: D[i0]
            run = None                                                  # (value at the current column, key, span)
            zl = feed
            out = None
            for x in range(i0 + 1, hi + 1):
                m, av, bv = M[r + x], A[r + x], B[r + x]
                ms = D[x - 1] if m > 0 else (x, y)
                a_free = no_end and x == la
                as_ = ((D[x] if a_free else V[x]) if av > 0 else (x, y))
                if forced:
                    bs = (x, y)
                else:
                    # candidates meet only as (left, right); between such two the right one wins a tie unless it is an
                    # opening from M -- one bit, nm, stands for the whole ordered key (sa_span.hip's header)
                    def merge(l, r):
                        return l if l[0] >= r[0] + r[1] else r
                    pos = x - i0 - 1
                    step = 0 if free_row else ext
                    w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"])
                    if not free_row and ext > 0 and 0 >= w[0]:
                        w = (0, 1, (x, y))                              # the floor of this very cell
                    if pos == 0:
                        w = merge((feed["b"] + step, 1, feed["bs"]), w)
                    if run is not None:
                        w = merge((run[0] + step, run[1], run[2]), w)
                    run = w
                    assert max(run[0], 0) == bv, (x, y, run, bv)
                    bs = run[2] if bv > 0 else (x, y)
                from_a = av >= m
                zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
                mb = max(m, bv)
                low = bs if bv >= m else ms
                nD[x] = as_ if av >= mb else low
                nV[x] = as_ if av + ext >= mb + open1 else low
                if m > col_best[x]:
                    col_best[x], col_info[x] = m, ((x, y), ms)
                out = dict(z=zl["z"], b=bv, from_a=from_a, zs=zl["zs"], bs=bs)
            if hi < la:                                                 # what this strip hands the next one
                feed = out
                zwins = (feed["z"] >= feed["b"]) if feed["from_a"] else (feed["z"] > feed["b"])
                assert nD[hi] == (feed["zs"] if zwins else feed["bs"]), (hi, y)
        D, V = nD, nV
    for x in range(1, W):
        if col_best[x] > best:
            best, (best_at, best_span) = col_best[x], col_info[x]
    return _fields(best, best_at, best_span)


# ----------------------------------------------------------------------------------------------- wide and tie-dense pairs ---
def best_cell_np(M, la: int):
    """best_cell on the oracle's int32 array: score descending, column ascending, row ascending."""
    M2 = np.asarray(M).reshape(-1, la + 1)
    best = int(M2.max())
    if best <= 0:
        return 0, None
    x = int(np.nonzero((M2 == best).any(axis=0))[0][0])
    return best, (x, int(np.nonzero(M2[:, x] == best)[0][0]))


def walk_both(osc, a: bytes, b: bytes):
    """(walk_span with WALKER, walk_span with REVERSED) of one pair, as plain ints.  The walks touch len_a + len_b cells, so
    the matrices stay numpy arrays and the best cell comes from numpy: a pair of 1 600 x 700 takes milliseconds."""
    rc, M, A, B = O.oracle_fill(osc, a, b, 1)
    assert rc == 0
    best = best_cell_np(M, len(a))
    return tuple(tuple(int(v) for v in walk_span(osc, a, b, pr, (M, A, B), best)) for pr in (WALKER, REVERSED))


def crosses_seam(span, seam: int = 512) -> bool:
    """Whether the hit's columns pos_a .. pos_a + len_a strictly contain a multiple of `seam` (a strip seam of sa_span.hip)."""
    _, pos_a, _, len_a, _ = span
    return any(pos_a < s < pos_a + len_a for s in range(seam, pos_a + len_a, seam))


TIE_SCORINGS = {"open0": [2, -1, 0, -1], "ext0": [3, -1, -1, 0], "ext_pos": [2, -3, -2, 1]}     # ext_pos: the only one whose floor pays
TIE_ROWS_WIDTHS = (200, 300, 400, 512)        # 4, 5, 8 and 8 columns per lane (1 .. 3: test_ties_follow_the_walkers_order)
TIE_STRIPS_WIDTHS = (700, 1100, 1600)         # two, three and four strips
# (scoring, width) -> seed where the default seed's pairs fall short of a share test_span_band_dense_argument_cpu.py asks for
# (open0 is the sparsest: seeds 1 .. 8 give 3 .. 10 tie-sensitive pairs of 40 and 9 .. 16 seam-crossing hits per strips width)
TIE_SEEDS = {("open0", 700): 4, ("open0", 1100): 6, ("open0", 1600): 6}


def indel_relative(rng, s: bytes, alpha: bytes) -> bytes:
    """One letter in twelve deleted, one in twelve preceded by 1 .. 3 inserted letters."""
    out = bytearray()
    for ch in s:
        r = rng.randrange(12)
        if r == 0:
            continue
        if r == 1:
            out += bytes(rng.choice(alpha) for _ in range(rng.randint(1, 3)))
        out.append(ch)
    return bytes(out)


def tie_pairs(name: str, width: int, n: int = 40, alpha: bytes = b"AC", seam: int = 512):
    """n pairs over a binary alphabet, len_a within 6 of `width` (one class of the span launcher), len_b <= 140; every second
    pair related by indels; for widths of several strips every second RELATED pair's seq_b comes from a stretch of seq_a that
    straddles a multiple of `seam`."""
    rng = random.Random(TIE_SEEDS.get((name, width), 1000 * len(name) + width))
    pairs = []
    for k in range(n):
        la = width - rng.randrange(7)
        a = bytes(rng.choice(alpha) for _ in range(la))
        if k % 2 == 0:
            b = bytes(rng.choice(alpha) for _ in range(rng.randint(1, 140)))
        else:
            L = rng.randint(40, 130)
            if width > seam and k % 4 == 3:
                s = seam * rng.randint(1, (la - 1) // seam)
                start = max(0, min(la - L, s - rng.randint(L // 4, 3 * L // 4)))
            else:
                start = rng.randrange(la - L + 1)
            b = indel_relative(rng, a[start:start + L], alpha)[:140]
        pairs.append((a, b))
    return pairs


FLAG_WIDTHS = (513, 700, 1025, 1100, 1537)


def flag_spec(no_gaps_in_a=0, no_gaps_in_b=0, no_mismatches=0, no_start=0, no_end=0):
    """test_all_flag_combinations_vs_oracle's scoring: mismatch -6 where both no-gaps flags are set."""
    return {"init": [1, -6 if (no_gaps_in_a and no_gaps_in_b) else -2, -4, -1, no_start, no_end, no_gaps_in_a, no_gaps_in_b, no_mismatches, 0]}


def _relative(rng, s: bytes, alpha: bytes = b"ACGT", keep: int = 15) -> bytes:
    """Substitutions, insertions and deletions at about one position in ten; the last `keep` letters stay as they are."""
    out = bytearray()
    for i, ch in enumerate(s):
        r = rng.randrange(30) if i < len(s) - keep else 17
        if r == 0:
            continue
        if r == 1:
            out += bytes(rng.choice(alpha) for _ in range(rng.randint(1, 3)))
        out.append(rng.choice(alpha) if r == 2 else ch)
    return bytes(out)


def flag_pairs(width: int, alpha: bytes = b"ACGT"):
    """Four pairs of len_a = width: seq_b a relative of seq_a's last 90 letters (the hit reaches the last column), of its first
    90 letters (unchanged at their end: the hit ends on the last row), of 90 letters around its middle, and unrelated."""
    rng = random.Random(31 * width)
    a = bytes(rng.choice(alpha) for _ in range(width))
    mid = width // 2 - 45
    return [(a, _relative(rng, a[-90:])), (a, _relative(rng, a[:90])), (a, _relative(rng, a[mid:mid + 90])),
            (a, bytes(rng.choice(alpha) for _ in range(90)))]


# ------------------------------------------------------------------------------------------------ ties AT a strip seam ---
# The right strip of sa_span.hip takes the predecessor of its first column's match cell from the left strip's hand-off:
# {max(M, A), B, whether A}.  Where gap_a and gap_b of the seam column tie for the maximum, A > B is decided by that one bit
# (`zwins`, `out.from_a`).  A pair tells a wrong bit only if its hit crosses the seam diagonally out of such a cell AND the two
# states' walks end in different cells.
SEAM_MUTANT = (GAP_B, GAP_A, MATCH)           # what the walk does at the seam if the bit is lost: B wins the tie
SEAM_SCORINGS = {"open0": [2, -1, 0, -1], "ext0": [3, -1, -1, 0], "swdense": [5, -10, 0, -1], "ties": [1, 0, 0, 0], "ext_pos": [2, -3, -2, 1]}
SEAM_WIDTHS = {name: ((513, 1025, 1537) if name == "ext_pos" else (700, 1100, 1600)) for name in SEAM_SCORINGS}
SEAM_N = 24


def walk_seams(osc, a: bytes, b: bytes, seam: int = 512):
    """(the walker's span, the span with SEAM_MUTANT on the diagonal steps across a seam, the same on the horizontal steps)."""
    rc, M, A, B = O.oracle_fill(osc, a, b, 1)
    assert rc == 0
    best = best_cell_np(M, len(a))
    walk = lambda **kw: tuple(int(v) for v in walk_span(osc, a, b, WALKER, (M, A, B), best, seam=seam, **kw))
    return walk(), walk(seam_priority=SEAM_MUTANT, seam_steps=(MATCH,)), walk(seam_priority=SEAM_MUTANT, seam_steps=(GAP_B,))


def seam_pairs(name: str, width: int, n: int = SEAM_N, seam: int = 512):
    """Pairs whose hit leaves a seam column diagonally out of a cell where gap_a and gap_b tie.
    ext_pos (a gap that pays): random DNA, len_a = width, one column past a seam -- the runs that pay meet at the row's end.
    The others: seq_a = filler S2 S1 | Q filler, seq_b = S1 S2 Q with `|` on a seam and S1, S2, Q over alphabets that share
    no letter: S1 matched and S2 skipped in seq_b (gap_a) scores what S2 matched and S1 skipped in seq_a (gap_b) does when
    the two are equally long (three pairs in four; the rest differ by one letter and do not tie), and the two walks start in
    different cells."""
    rng = random.Random(7 * width + len(name))
    seg = lambda k, alpha: bytes(rng.choice(alpha) for _ in range(k))
    pairs = []
    for k in range(n):
        if name == "ext_pos":
            pairs.append((seg(width, b"ACGT"), seg(rng.randint(20, 140), b"ACGT")))
            continue
        s = seam * (1 + k % ((width - 1) // seam))
        L2 = rng.randint(6, 40)
        L1 = L2 + (rng.choice([-1, 1]) if k % 4 == 3 else 0)
        S1, S2, Q = seg(L1, b"CG"), seg(L2, b"TW"), seg(rng.randint(10, 50), b"KMRY")
        a = b"A" * (s - L1 - L2) + S2 + S1 + Q
        pairs.append((a + b"A" * (width - rng.randrange(7) - len(a)), S1 + S2 + Q))
    return pairs
