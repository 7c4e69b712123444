"""Helpers of the SW alignment-statistics tests (seqalign_sw_stats_batch / _cross).  Not a test module.

want_sw_stats       what the calls must return, from the oracle's first hit (orclib.oracle_sw, min_score = 1, max_hits = 1):
                    (score, pos_a, pos_b, len_a, len_b, matches, mismatches) per pair, the counts those of the hit's strings
                    (statlib.count_columns); seven zeros where there is no hit;
hit_fields          the same seven values from a hit dict of sw_batch / sw_align_long;
forward             the DEFINITION the kernel rests on, in pure Python over the oracle's matrices: spanlib.propagate
                    with counts beside the span -- the payload of (cell, state) is (the cell itself, 0, 0) where the value is <= 0
                    or the cell is on the border, else the payload of the predecessor alignment_reverse_move picks, plus one match
                    or mismatch for a match state's own letters;
walk                the same by walking back from the best cell: one path instead of all cells (numpy matrices welcome);
pack_cell ...       the kernel's two payload words, as Python ints masked to 32 bits: x | y << 16 and matches | mismatches << 16;
kernel_model        the kernel's own shape on the CPU IN PACKED FORM: two merged payloads per column across rows, the running
                    maximum along a row under the one-bit tie rule, strips that hand on {max(M, A), B, whether A's, two payloads},
                    the running best per column -- values from the oracle, payloads carried as the two packed words -- checked
                    state by state against `forward`;
tie_sensitive       how many pairs change their counts under M > B > A;
planted             a pair whose only hit is one planted stretch.
"""
from __future__ import annotations

import denselib as D  # noqa: F401  (the GPU tests take the gap-dense families from here)
import orclib as O
import spanlib as SP
import statlib as ST

MATCH, GAP_A, GAP_B = O.MATCH, O.GAP_A, O.GAP_B
WALKER, REVERSED = SP.WALKER, SP.REVERSED
MAX_LEN = 65535                # SEQALIGN_SW_STATS_MAX_LEN
MASK = 0xFFFFFFFF
ZEROS = (0, 0, 0, 0, 0, 0, 0)


def hit_fields(osc, hits):
    """The seven values of a list of at most one hit dict (orclib.oracle_sw's, Context.sw_batch's, Context.sw_align_long's): the
    hit's fields and the counted columns of its strings, which come back as str."""
    if not hits:
        return ZEROS
    h = hits[0]
    return (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) + ST.count_columns(osc, h["a"].encode(), h["b"].encode())


def want_one(osc, a: bytes, b: bytes):
    rc, hits = O.oracle_sw(osc, a, b, 1, 1)
    assert rc == 0, rc
    return hit_fields(osc, hits)


def want_sw_stats(osc, pairs):
    """[(score, pos_a, pos_b, len_a, len_b, matches, mismatches)] per (a, b)."""
    return [want_one(osc, a, b) for a, b in pairs]


def got_sw_stats(res):
    """sw_stats' seven arrays as the list want_sw_stats returns."""
    return [tuple(int(x[p]) for x in res) for p in range(len(res[0]))]


def _fields(best, at, payload):
    if best <= 0:
        return ZEROS
    (x0, y0), m, mm = payload
    return (best, x0, y0, at[0] - x0, at[1] - y0, m, mm)


def _penalties(osc, x, y, la, lb):
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    a_open, a_ext, b_open, b_ext = open1, ext, open1, ext          # alignment.c:261-272
    if osc.no_end_gap_penalty:
        if x == la:
            a_open = a_ext = 0
        if y == lb:
            b_open = b_ext = 0
    return a_open, a_ext, b_open, b_ext


def forward(osc, a: bytes, b: bytes, priority=WALKER, mats=None):
    """Returns (result, pay): result = the seven values; pay[state][y * W + x] = ((x0, y0), matches, mismatches)."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = mats or SP._matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = SP._Lookup(osc)
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)
    pay = {st: [None] * (W * (lb + 1)) for st in (MATCH, GAP_A, GAP_B)}
    for y in range(lb + 1):
        for x in range(W):
            at = y * W + x
            for st in (MATCH, GAP_A, GAP_B):
                v = vals[st][at]
                if v <= 0 or x == 0 or y == 0:
                    pay[st][at] = ((x, y), 0, 0)
                    continue
                a_open, a_ext, b_open, b_ext = _penalties(osc, x, y, la, lb)
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
                        stop, m, mm = pay[s2][pat]
                        break
                else:
                    raise SP.NoPredecessor((x, y, st))
                if st == MATCH:
                    eq = fa[x - 1] == fb[y - 1]
                    m, mm = m + eq, mm + (not eq)
                pay[st][at] = (stop, m, mm)
    best, at = SP.best_cell(M, la, lb)
    return _fields(best, at, pay[MATCH][at[1] * W + at[0]] if at else None), pay


def walk(osc, a: bytes, b: bytes, priority=WALKER, mats=None, best=None):
    """The seven values by WALKING back from the best cell with the given priority, counting the letter columns it emits."""
    la, lb = len(a), len(b)
    W = la + 1
    if mats is None:
        rc, *mats = O.oracle_fill(osc, a, b, 1)
        assert rc == 0
    M, A, B = mats
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = SP._Lookup(osc)
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)
    best, at = best or SP.best_cell_np(M, la)
    if best <= 0:
        return ZEROS
    (x, y), st, v = at, MATCH, best
    m = mm = 0
    while v > 0 and x > 0 and y > 0:
        a_open, a_ext, b_open, b_ext = _penalties(osc, x, y, la, lb)
        if st == MATCH:
            eq = fa[x - 1] == fb[y - 1]
            m, mm = m + eq, mm + (not eq)
            s = look(a[x - 1], b[y - 1])
            via, x, y = {MATCH: s, GAP_A: s, GAP_B: s}, x - 1, y - 1
        elif st == GAP_A:
            via, y = {MATCH: a_open, GAP_A: a_ext, GAP_B: a_open}, y - 1
        else:
            via, x = {MATCH: b_open, GAP_A: b_open, GAP_B: b_ext}, x - 1
        pat = y * W + x
        ok = {GAP_A: (not osc.no_gaps_in_a) or x == 0 or x == la, GAP_B: (not osc.no_gaps_in_b) or y == 0 or y == lb, MATCH: True}
        for s2 in priority:
            if ok[s2] and int(vals[s2][pat]) + via[s2] == v:
                st, v = s2, int(vals[s2][pat])
                break
        else:
            raise SP.NoPredecessor((x, y, st))
    return _fields(int(best), at, ((x, y), int(m), int(mm)))


def tie_sensitive(osc, pairs) -> int:
    """Pairs whose (matches, mismatches) change when the predecessor priority is reversed to M > B > A."""
    n = 0
    for a, b in pairs:
        rc, M, A, B = O.oracle_fill(osc, a, b, 1)
        assert rc == 0
        best = SP.best_cell_np(M, len(a))
        n += walk(osc, a, b, WALKER, (M, A, B), best)[5:] != walk(osc, a, b, REVERSED, (M, A, B), best)[5:]
    return n


# ------------------------------------------------------------------------------------------------- the packed words ---
def pack_cell(x: int, y: int) -> int:
    return (x | (y << 16)) & MASK


def unpack_cell(w0: int):
    return w0 & 0xFFFF, w0 >> 16


def pack_counts(m: int, mm: int) -> int:
    return (m | (mm << 16)) & MASK


def unpack_counts(w1: int):
    return w1 & 0xFFFF, w1 >> 16


def count_step(w1: int, eq: bool) -> int:
    """A match state's own letters: ONE 32-bit add of 1 or 0x10000."""
    return (w1 + (1 if eq else 0x10000)) & MASK


def unpacked(words):
    return (unpack_cell(words[0]),) + unpack_counts(words[1])


def kernel_model(osc, a: bytes, b: bytes, strip_cols: int = 1 << 30, pay=None):
    """The seven values the way the kernel finds them, payloads as (word 0, word 1).  pay: forward()'s payloads -- every state of
    every cell is then compared with the definition."""
    la, lb = len(a), len(b)
    assert la <= MAX_LEN and lb <= MAX_LEN
    W = la + 1
    M, A, B = SP._matrices(osc, a, b)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, no_gaps_b = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_b)
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)
    D_ = [(pack_cell(x, 0), 0) for x in range(W)]          # row 0
    V = list(D_)
    col_best = [0] * W
    col_info = [None] * W

    def merge(l, r):                       # l lies left of r: r wins a tie unless it is an opening from M (nm = 0)
        return l if l[0] >= r[0] + r[1] else r

    for y in range(1, lb + 1):
        r = y * W
        free_row, forced = no_end and y == lb, no_gaps_b and y != lb
        edge = (pack_cell(0, y), 0)
        nD, nV = [edge] + [None] * la, [edge] + [None] * la
        feed = dict(z=0, b=0, from_a=False, zs=edge, bs=edge)      # the border column
        for i0 in range(0, max(la, 1), strip_cols):
            hi = min(la, i0 + strip_cols)
            run, zl, out = None, feed, None
            for x in range(i0 + 1, hi + 1):
                m, av, bv = M[r + x], A[r + x], B[r + x]
                here = (pack_cell(x, y), 0)
                ms = (D_[x - 1][0], count_step(D_[x - 1][1], fa[x - 1] == fb[y - 1])) if m > 0 else here
                a_free = no_end and x == la
                as_ = ((D_[x] if a_free else V[x]) if av > 0 else here)
                if forced:
                    bs = here
                else:
                    step = 0 if free_row else ext
                    w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"])
                    if not free_row and ext > 0 and 0 >= w[0]:
                        w = (0, 1, here)                                # the floor of this very cell
                    if x == i0 + 1:
                        w = merge((feed["b"] + step, 1, feed["bs"]), w)
                    if run is not None:
                        w = merge((run[0] + step, run[1], run[2]), w)
                    run = w
                    assert max(run[0], 0) == bv, (x, y, run, bv)
                    bs = run[2] if bv > 0 else here
                if pay is not None:
                    for st, got in ((MATCH, ms), (GAP_A, as_), (GAP_B, bs)):
                        assert unpacked(got) == pay[st][r + x], (st, x, y, unpacked(got), pay[st][r + x])
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
        D_, V = nD, nV
    best, best_at, words = 0, None, None
    for x in range(1, W):
        if col_best[x] > best:
            best, (best_at, words) = col_best[x], col_info[x]
    if best <= 0:
        return ZEROS
    u64 = (words[0] << 32) | words[1]                                   # reduce_best's one word, and the write's unpacking
    w0, w1 = u64 >> 32, u64 & MASK
    return _fields(best, best_at, (unpack_cell(w0),) + unpack_counts(w1))


def planted(rng, la: int, lb: int, at_a: int, at_b: int, length: int, alpha: bytes = b"ACGT", other: bytes = b"KMRY"):
    """A pair of la x lb letters over alphabets that share nothing, with one common stretch of `length` letters (a few of them
    substituted) at seq_a[at_a:] and seq_b[at_b:]: the only hit."""
    a = bytearray(rng.choice(alpha[:2]) for _ in range(la))
    b = bytearray(rng.choice(other) for _ in range(lb))
    core = bytes(rng.choice(alpha[2:] + b"W") for _ in range(length))
    a[at_a:at_a + length] = core
    core_b = bytearray(core)
    for k in range(7, length - 7, 23):
        core_b[k] = other[0]
    b[at_b:at_b + length] = core_b
    return bytes(a), bytes(b)
