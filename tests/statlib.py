"""Helpers of the NW alignment-statistics tests (seqalign_nw_stats_batch / _cross).  Not a test module.

count_columns       (matches, mismatches) of two alignment strings, letters compared after the scoring's own case folding;
want_stats          what the calls must return, counted from orclib.oracle_nw's strings: (score, matches, mismatches) per pair,
                    None for a pair whose traceback fails;
step                one alignment_reverse_move over the oracle's matrices, priority selectable: the predecessor or None;
forward             the DEFINITION the kernel rests on, in pure Python over the oracle's matrices: the counts
                    of (cell, state) are (0, 0) on the border, else the counts of the predecessor the walker picks (plus one
                    for a match state's own letters), a state without a predecessor carries a sticky "no walk" mark;
walk                the same by walking back from the end pick: one path instead of all cells;
kernel_model        the kernel's own shape on the CPU: two merged payloads per column across rows, the running maximum along a
                    row under the one-bit tie rule, strips that hand on {max(M, A), B, whether A's, two payloads} -- payloads
                    only, values from the oracle -- checked cell by cell against `forward`;
tie_pairs           the tie-dense pairs of one width; tie_sensitive: how many change their counts under M > B > A.
"""
from __future__ import annotations

import ctypes as C
import random

import numpy as np

import orclib as O
import spanlib as SP

MATCH, GAP_A, GAP_B = O.MATCH, O.GAP_A, O.GAP_B
WALKER, REVERSED = SP.WALKER, SP.REVERSED
NO_WALK = "no walk"
E_UNKNOWN_PAIR, E_TRACEBACK = 5, 7


def floor_of(osc) -> int:
    """The NW floor (alignment.c:41)."""
    return -(1 << 31) + abs(osc.min_penalty)


def fold(osc, s: bytes) -> bytes:
    return s if osc.case_sensitive else s.lower()


def count_columns(osc, ra: bytes, rb: bytes):
    """(matches, mismatches) over the columns that hold a letter of both strings."""
    fa, fb = np.frombuffer(fold(osc, ra), np.uint8), np.frombuffer(fold(osc, rb), np.uint8)
    both = (np.frombuffer(ra, np.uint8) != 45) & (np.frombuffer(rb, np.uint8) != 45)
    m = int(np.count_nonzero(both & (fa == fb)))
    return m, int(np.count_nonzero(both)) - m


def want_one(osc, a: bytes, b: bytes):
    rc, s, ra, rb = O.oracle_nw(osc, a, b)
    if rc:
        return None if rc == E_TRACEBACK else ("rc", rc)
    return (s,) + count_columns(osc, ra, rb)


def want_stats(osc, pairs):
    """[(score, matches, mismatches) | None] per (a, b)."""
    return [want_one(osc, a, b) for a, b in pairs]


def got_stats(res):
    """nw_stats' three arrays as the list want_stats returns."""
    return [tuple(int(x[p]) for x in res) for p in range(len(res[0]))]


class Lookup:
    """scoring_lookup of the oracle, one call per distinct character pair: (score, is_match)."""

    def __init__(self, osc):
        self.osc, self.memo, self.lib = osc, {}, O.oracle()

    def __call__(self, ca: int, cb: int):
        k = (ca, cb)
        if k not in self.memo:
            s, m = C.c_int(0), C.c_int(0)
            rc = self.lib.orc_scoring_lookup(C.byref(self.osc), C.c_char(bytes([ca])), C.c_char(bytes([cb])), C.byref(s), C.byref(m))
            assert rc == 0, (ca, cb)
            self.memo[k] = (s.value, bool(m.value))
        return self.memo[k]


def matrices(osc, a, b, as_lists=True):
    rc, M, A, B = O.oracle_fill(osc, a, b, 0)
    assert rc == 0
    return (M.tolist(), A.tolist(), B.tolist()) if as_lists else (M, A, B)


def end_pick(M, A, B, at):
    """needleman_wunsch.c:53-66: M, then B if B >= M, then A if A >= that."""
    st, v = MATCH, M[at]
    if B[at] >= v:
        st, v = GAP_B, B[at]
    if A[at] >= v:
        st, v = GAP_A, A[at]
    return st, int(v)


def step(osc, vals, a, b, x, y, st, look, priority=WALKER):
    """alignment_reverse_move from state st of cell (x, y), x > 0 and y > 0: (state, x', y') it moves to, or None where no
    predecessor satisfies its equality (the reference exits there: SEQALIGN_E_TRACEBACK)."""
    la, lb = len(a), len(b)
    W = la + 1
    v = vals[st][y * W + x]
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    a_open, a_ext, b_open, b_ext = open1, ext, open1, ext          # alignment.c:261-272 (x, y > 0: no_start plays no part)
    if osc.no_end_gap_penalty:
        if x == la:
            a_open = a_ext = 0
        if y == lb:
            b_open = b_ext = 0
    if st == MATCH:
        s = look(a[x - 1], b[y - 1])[0]
        via, nx, ny = {MATCH: s, GAP_A: s, GAP_B: s}, x - 1, y - 1
    elif st == GAP_A:
        via, nx, ny = {MATCH: a_open, GAP_A: a_ext, GAP_B: a_open}, x, y - 1
    else:
        via, nx, ny = {MATCH: b_open, GAP_A: b_open, GAP_B: b_ext}, x - 1, y
    pat = ny * W + nx
    ok = {GAP_A: (not osc.no_gaps_in_a) or nx == 0 or nx == la, GAP_B: (not osc.no_gaps_in_b) or ny == 0 or ny == lb, MATCH: True}
    for s2 in priority:
        if ok[s2] and int(vals[s2][pat]) + via[s2] == v:
            return s2, nx, ny
    return None


def forward(osc, a: bytes, b: bytes, priority=WALKER, mats=None, blocked_marks=True):
    """The forward definition.  blocked_marks: the match state of a cell whose letters no_mismatches blocks has no predecessor
    (the definition); False asks the walker there too, which looks such a pair up as score 0 and so steps into any admitted
    state that holds exactly the floor (test_nw_stats_argument_cpu.py shows the one family where the two differ).
    Returns (result, cnt, bsrc): result = (score, matches, mismatches) or NO_WALK;
    cnt[state][y * W + x] = (matches, mismatches, marked); bsrc[y * W + x] = where the walk from gap_b of that cell leaves the
    row's chain, found step by step: ('A' | 'M', k) an opening out of column k - 1, ('F', k) no predecessor at column k,
    ('L', 0) the border column."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = mats or matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = Lookup(osc)
    fa, fb = fold(osc, a), fold(osc, b)
    cnt = {st: [(0, 0, False)] * (W * (lb + 1)) for st in (MATCH, GAP_A, GAP_B)}
    bsrc = [("L", 0)] * (W * (lb + 1))
    for y in range(1, lb + 1):
        for x in range(1, W):
            at = y * W + x
            for st in (MATCH, GAP_A, GAP_B):
                pred = step(osc, vals, a, b, x, y, st, look, priority)
                if st == MATCH and blocked_marks and osc.no_mismatches and not look(a[x - 1], b[y - 1])[1]:
                    pred = None
                if pred is None:
                    cnt[st][at] = (0, 0, True)
                    if st == GAP_B:
                        bsrc[at] = ("F", x)
                    continue
                s2, nx, ny = pred
                m, mm, mark = cnt[s2][ny * W + nx]
                if st == MATCH:
                    eq = fa[x - 1] == fb[y - 1]
                    m, mm = m + eq, mm + (not eq)
                elif st == GAP_B:
                    bsrc[at] = bsrc[at - 1] if s2 == GAP_B else ("A" if s2 == GAP_A else "M", x)
                cnt[st][at] = (m, mm, mark)
    st, score = end_pick(M, A, B, W * (lb + 1) - 1)
    m, mm, mark = cnt[st][W * (lb + 1) - 1]
    return (NO_WALK if mark else (score, m, mm)), cnt, bsrc


def walk(osc, a: bytes, b: bytes, priority=WALKER, mats=None):
    """(score, matches, mismatches) or NO_WALK by walking back from the end pick with the given priority."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = mats or matrices(osc, a, b, as_lists=False)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = Lookup(osc)
    fa, fb = fold(osc, a), fold(osc, b)
    st, score = end_pick(M, A, B, W * (lb + 1) - 1)
    x, y, m, mm = la, lb, 0, 0
    while x > 0 and y > 0:
        if st == MATCH:
            eq = fa[x - 1] == fb[y - 1]
            m, mm = m + eq, mm + (not eq)
        pred = step(osc, vals, a, b, x, y, st, look, priority)
        if pred is None:
            return NO_WALK
        st, x, y = pred
    return (score, m, mm)


def kernel_model(osc, a: bytes, b: bytes, strip_cols: int = 1 << 30, fw=None):
    """(score, matches, mismatches) or NO_WALK the way the kernel finds it.  fw: forward()'s (cnt, bsrc) -- every state a walk
    can stand in is then compared with the definition, and every gap_b cell's source with the step-by-step walk."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = matrices(osc, a, b)
    st, score = end_pick(M, A, B, W * (lb + 1) - 1)
    if la == 0 or lb == 0:
        return (score, 0, 0)
    fl = floor_of(osc)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, nga, ngb, no_mm = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_a), bool(osc.no_gaps_in_b), bool(osc.no_mismatches)
    look = Lookup(osc)
    fa, fb = fold(osc, a), fold(osc, b)
    Z, MARK = (0, 0, False), (0, 0, True)
    D, V = [Z] * W, [Z] * W                # row 0: a walk that reaches it has counted everything

    def merge(l, r):                       # l lies left of r: r wins a tie only as an opening from A (nm = 1)
        return l if l[0] >= r[0] + r[1] else r

    for y in range(1, lb + 1):
        r = y * W
        free_row, forced = no_end and y == lb, ngb and y != lb
        nD, nV = [Z] + [None] * la, [Z] + [None] * la
        feed = dict(z=max(M[r], A[r]), b=B[r], from_a=A[r] >= M[r], zs=Z, bs=Z, bsrc=("L", 0))      # the border column
        for i0 in range(0, la, strip_cols):
            hi = min(la, i0 + strip_cols)
            run, zl, out = None, feed, None
            for x in range(i0 + 1, hi + 1):
                m, av, bv = M[r + x], A[r + x], B[r + x]
                a_ok = (not nga) or x == la                            # gap_a of this column can be walked into
                pd, pu = r - W + x - 1, r - W + x
                s, is_match = look(a[x - 1], b[y - 1])
                eq = fa[x - 1] == fb[y - 1]
                if (no_mm and not is_match) or max(M[pd], A[pd], B[pd]) + s < fl:
                    ms = MARK
                else:
                    ms = (D[x - 1][0] + eq, D[x - 1][1] + (not eq), D[x - 1][2])
                if no_end and x == la:
                    as_ = D[x]
                elif not a_ok or max(max(M[pu], B[pu]) + open1, A[pu] + ext) < fl:
                    as_ = MARK
                else:
                    as_ = V[x]
                if forced:
                    bs, bsrc = MARK, ("F", x)
                else:
                    step_ = 0 if free_row else ext
                    w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"], ("A" if zl["from_a"] else "M", x))
                    if not free_row and fl > w[0]:
                        w = (fl, 0, MARK, ("F", x))                    # clamped: the floor loses a tie to every candidate
                    if x == i0 + 1:
                        w = merge((feed["b"] + step_, 1, feed["bs"], feed["bsrc"]), w)
                    if run is not None:
                        w = merge((run[0] + step_, run[1], run[2], run[3]), w)
                    run = w
                    assert run[0] == bv, (x, y, run, bv)
                    bs, bsrc = run[2], run[3]
                if fw is not None:
                    cnt, src = fw
                    assert cnt[MATCH][r + x] == ms, ("M", x, y)
                    if a_ok:
                        assert cnt[GAP_A][r + x] == as_, ("A", x, y)
                    if not forced:
                        assert cnt[GAP_B][r + x] == bs, ("B", x, y)
                        assert src[r + x] == bsrc, ("B source", x, y, src[r + x], bsrc)
                from_a = a_ok and av >= m
                zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
                mb = max(m, bv)
                low = bs if (not forced and bv >= m) else ms
                nD[x] = as_ if (a_ok and av >= mb) else low
                nV[x] = as_ if (a_ok and av + ext >= mb + open1) else low
                out = dict(z=zl["z"], b=bv, from_a=from_a, zs=zl["zs"], bs=bs, bsrc=bsrc)
            if hi < la:                                                 # what this strip hands the next one
                feed = out
                zwins = forced or ((feed["z"] >= feed["b"]) if feed["from_a"] else (feed["z"] > feed["b"]))
                assert nD[hi] == (feed["zs"] if zwins else feed["bs"]), (hi, y)
        D, V = nD, nV
    m, mm, mark = D[la]
    return NO_WALK if mark else (score, m, mm)


# ----------------------------------------------------------------------------------------------------- tie-dense pairs ---
TIE_SCORINGS = {"ext0": [3, -1, -1, 0], "ties": [1, 0, 0, 0], "ext_pos": [2, -3, -2, 1]}
TIE_WIDTHS = (64, 200, 512, 700, 1100)
TIE_MIN = 10          # of 40 pairs
# (scoring, width) -> seed where the default seed's pairs fall short of TIE_MIN
TIE_SEEDS: dict = {}


def tie_pairs(name: str, width: int, n: int = 40, alpha: bytes = b"AC"):
    """n pairs over a binary alphabet, len_a within 6 of `width`; every second pair an indel relative of seq_a, the others
    random with len_b in [len_a / 2, len_a]."""
    rng = random.Random(TIE_SEEDS.get((name, width), 2000 * len(name) + width))
    pairs = []
    for k in range(n):
        la = max(1, width - rng.randrange(7))
        a = bytes(rng.choice(alpha) for _ in range(la))
        if k % 2:
            b = SP.indel_relative(rng, a, alpha)
        else:
            b = bytes(rng.choice(alpha) for _ in range(rng.randint(la // 2, la)))
        pairs.append((a, b))
    return pairs


def tie_sensitive(osc, pairs) -> int:
    """Pairs whose (matches, mismatches) change when the predecessor priority is reversed to M > B > A (the end pick stays)."""
    n = 0
    for a, b in pairs:
        mats = matrices(osc, a, b, as_lists=False)
        n += walk(osc, a, b, WALKER, mats) != walk(osc, a, b, REVERSED, mats)
    return n


def init_spec(init4, no_start=0, no_end=0, no_gaps_in_a=0, no_gaps_in_b=0, no_mismatches=0, case_sensitive=0):
    return {"init": [*init4, no_start, no_end, no_gaps_in_a, no_gaps_in_b, no_mismatches, case_sensitive]}
