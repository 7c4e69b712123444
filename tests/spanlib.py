"""Helpers of the SW hit-span tests (seqalign_sw_span_batch).  Not a test module.

want_spans          what the call must return, from the oracle's first hit (orclib.oracle_sw, min_score = 1, max_hits = 1);
propagate           the DEFINITION the kernel rests on, in pure Python over the oracle's matrices: the span of (cell, state) is
                    the cell itself where the value is <= 0 or the cell is on the border, else the span of the predecessor
                    alignment_reverse_move picks (priority selectable);
gap_b_sources       along a row, the source of every gap_b cell by the walker's sequential rule and by the ordered-key rule;
kernel_model        the kernel's own shape on the CPU: two merged spans per column across rows, the running maximum along a
                    row with the kernel's one-bit tie rule, strips that hand on {max(M, A), B, whether A, two spans} -- spans only, values from the oracle;
walk_span           the first hit by walking back from the best cell with a selectable priority;
tie_sensitive       how many pairs of a batch change their span when the priority is reversed to M > B > A.
"""
from __future__ import annotations

import ctypes as C

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


def walk_span(osc, a: bytes, b: bytes, priority=WALKER, mats=None):
    """(score, pos_a, pos_b, len_a, len_b) of the first hit by WALKING back from the best cell with the given priority: what
    the propagation gives for that priority (test_sw_span_argument_cpu.py), at the cost of one path instead of all cells."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = mats or _matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    look = _Lookup(osc)
    best, at = best_cell(M, la, lb)
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
        for s2 in priority:
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
