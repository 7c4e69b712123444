"""Helpers of the SW gap-run tests (seqalign_sw_gaps_batch / _banded / _banded_wide).  Not a test module.

gap_runs            the numbers of maximal runs of '-' in a hit's two strings;
want_gaps           what the unbanded call must return per pair, from the oracle's first hit (orclib.oracle_sw, min_score = 1,
                    max_hits = 1): (score, end_a, end_b, gap_runs_a, gap_runs_b), zeros without a hit;
band_want           the same over the banded matrices (bandswlib.expected): ((score, end_a, end_b) of the banded score call, the five);
host_gaps           the five of a hit dict of sw_batch / sw_align_long / sw_align_banded(_wide), its strings counted on the host;
got_gaps            sw_gaps' five arrays as a list of such tuples;
forward             the DEFINITION the kernels rest on, in pure Python over the oracle's matrices: run(cell, S) is
                    (0, 0) where the walk of alignment_reverse_move that starts in state S of the cell stops in that very cell
                    (value <= 0 or a border cell; over banded matrices a cell outside the band holds 0), else run(the predecessor
                    the walker picks), plus one in a gap state's own word UNLESS the picked predecessor is the same gap state and
                    is not itself a stop.  The match state adds nothing;
walk                the same by walking back from the best cell; also says how many runs of the walk begin by EXTENDING out of
                    a stop (the runs an "open move" count misses);
naive_open_moves    a deliberately wrong model: one run per move from another state into a gap state;
kernel_model        the sweep's own shape on the CPU (sa_sw_gaps.hpp): swcountlib.kernel_model with the payload of a state two
                    plain Python ints (gap_runs_a, gap_runs_b); every feed, hand-off and stop RAW, the increment decided in the
                    consuming cell; strips hand on {max(M, A), B, whether A's, the two pairs};
frame_model         swcountlib.frame_model in the same form: the band frame's bookkeeping (sa_band_frame.hpp, sa_band_gaps.hip);
                    a position without a band cell carries POISON;
gap_rich_pairs      small pairs with an insertion and a deletion each;
deleted_block       the constructed long pair: a sequence against itself with one block deleted.
"""
from __future__ import annotations

import bandspanlib as BSP
import bandswlib as BS
import orclib as O
import spanlib as SP
import statlib as ST
import swstatlib as SS
from seqalign_amd import workloads as W

MATCH, GAP_A, GAP_B = SS.MATCH, SS.GAP_A, SS.GAP_B
WALKER, REVERSED = SP.WALKER, SP.REVERSED
ZEROS = (0, 0, 0, 0, 0)
POISON = None
STOP = (0, 0)                      # a state that stops has emitted no column, wherever it stops


def gap_runs(ra, rb):
    """(runs of '-' in string a, runs of '-' in string b); str or bytes."""
    def runs(s):
        s = s.decode() if isinstance(s, (bytes, bytearray)) else s
        return sum(1 for k, ch in enumerate(s) if ch == "-" and (k == 0 or s[k - 1] != "-"))
    return runs(ra), runs(rb)


def host_gaps(hits):
    """(score, end_a, end_b, gap_runs_a, gap_runs_b) of a list of at most one hit dict."""
    if not hits:
        return ZEROS
    h = hits[0]
    return (h["score"], h["pos_a"] + h["len_a"], h["pos_b"] + h["len_b"]) + gap_runs(h["a"], h["b"])


def want_one(osc, a: bytes, b: bytes):
    rc, hits = O.oracle_sw(osc, a, b, 1, 1)
    assert rc == 0, rc
    return host_gaps(hits)


def want_gaps(osc, pairs):
    return [want_one(osc, a, b) for a, b in pairs]


def band_want(osc, a: bytes, b: bytes, lo: int, hi: int):
    cell, hit = BS.expected(osc, a, b, lo, hi, 1)
    return tuple(cell), host_gaps([hit] if hit else [])


def got_gaps(res):
    return [tuple(int(x[p]) for x in res) for p in range(len(res[0]))]


# ------------------------------------------------------------------------------------------------- the definition ---
def _predecessor(osc, vals, look, a, b, x, y, st, v, la, lb, W_, priority):
    """(state, index, x, y) of the predecessor alignment_reverse_move picks for state st of cell (x, y) with value v."""
    a_open, a_ext, b_open, b_ext = SS._penalties(osc, x, y, la, lb)
    if st == MATCH:
        s = look(a[x - 1], b[y - 1])
        via, nx, ny = {MATCH: s, GAP_A: s, GAP_B: s}, x - 1, y - 1
    elif st == GAP_A:
        via, nx, ny = {MATCH: a_open, GAP_A: a_ext, GAP_B: a_open}, x, y - 1
    else:
        via, nx, ny = {MATCH: b_open, GAP_A: b_open, GAP_B: b_ext}, x - 1, y
    pat = ny * W_ + nx
    ok = {GAP_A: (not osc.no_gaps_in_a) or nx == 0 or nx == la, GAP_B: (not osc.no_gaps_in_b) or ny == 0 or ny == lb, MATCH: True}
    for s2 in priority:
        if ok[s2] and int(vals[s2][pat]) + via[s2] == v:
            return s2, pat, nx, ny
    raise SP.NoPredecessor((x, y, st))


def _bump(pair, st):
    return (pair[0] + 1, pair[1]) if st == GAP_A else (pair[0], pair[1] + 1)


def forward(osc, a: bytes, b: bytes, priority=WALKER, mats=None, naive=False):
    """Returns (five, pay): pay[state][y * W + x] = (gap_runs_a, gap_runs_b) of the walk that starts there.
    naive: the wrong rule -- a gap state adds one iff the picked predecessor is another state (an "open" move)."""
    la, lb = len(a), len(b)
    W_ = la + 1
    M, A, B = mats or SP._matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = SP._Lookup(osc)
    pay = {st: [None] * (W_ * (lb + 1)) for st in (MATCH, GAP_A, GAP_B)}
    for y in range(lb + 1):
        for x in range(W_):
            at = y * W_ + x
            for st in (MATCH, GAP_A, GAP_B):
                v = vals[st][at]
                if v <= 0 or x == 0 or y == 0:
                    pay[st][at] = STOP
                    continue
                s2, pat, nx, ny = _predecessor(osc, vals, look, a, b, x, y, st, v, la, lb, W_, priority)
                got = pay[s2][pat]
                if st != MATCH:
                    pred_stops = vals[s2][pat] <= 0 or nx == 0 or ny == 0
                    begins = (s2 != st) if naive else not (s2 == st and not pred_stops)
                    if begins:
                        got = _bump(got, st)
                pay[st][at] = got
    best, at = SP.best_cell(M, la, lb)
    if best <= 0:
        return ZEROS, pay
    return (best, at[0], at[1]) + pay[MATCH][at[1] * W_ + at[0]], pay


def naive_open_moves(osc, a: bytes, b: bytes, mats=None):
    return forward(osc, a, b, mats=mats, naive=True)[0]


def walk(osc, a: bytes, b: bytes, priority=WALKER, mats=None):
    """(five, runs that begin by extending out of a stop) by WALKING back from the best cell, counting a run where the walk
    leaves a gap state for anything but a live state of its own kind."""
    la, lb = len(a), len(b)
    W_ = la + 1
    M, A, B = mats or SP._matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = SP._Lookup(osc)
    best, at = SP.best_cell(M, la, lb)
    if best <= 0:
        return ZEROS, 0
    (x, y), st, v = at, MATCH, best
    runs, out_of_stop = (0, 0), 0
    while v > 0 and x > 0 and y > 0:
        s2, pat, nx, ny = _predecessor(osc, vals, look, a, b, x, y, st, v, la, lb, W_, priority)
        v2 = int(vals[s2][pat])
        if st != MATCH:
            pred_stops = v2 <= 0 or nx == 0 or ny == 0
            if not (s2 == st and not pred_stops):
                runs = _bump(runs, st)
                out_of_stop += s2 == st
        x, y, st, v = nx, ny, s2, v2
    return (int(best), at[0], at[1]) + runs, out_of_stop


# ---------------------------------------------------------------------------------------------- the kernel's shape ---
def _result(best, at, words):
    if best <= 0:
        return ZEROS
    assert 0 <= words[0] < 1 << 32 and 0 <= words[1] < 1 << 32
    u64 = (words[0] << 32) | words[1]                                   # reduce_best's one word, and the write's two halves
    return (best, at[0], at[1], u64 >> 32, u64 & SS.MASK)


def _gap_a_state(av, src, a_free, ap, yv, xv, open1, ext, gap_open):
    """gap_a's pair in the consuming cell: the raw feed + 1 unless the extension wins it and the gap_a above is > 0."""
    if av <= 0:
        return STOP
    ext_wins = ap >= yv if a_free else ap + ext >= yv + open1
    if gap_open <= 0 and not a_free:                        # the plain sweep keeps no max(M, B): it compares with max3 instead
        assert ext_wins == (ap + ext >= xv + open1)
    return src if (ext_wins and ap > 0) else (src[0] + 1, src[1])


def _merge(l, r):                      # l lies left of r: r wins a tie unless it is an opening from M (nm = 0)
    return l if l[0] >= r[0] + r[1] else r


def _gap_b_candidate(zl, feed, first, run, free_row, open1, ext):
    """The running candidate of the gap_b chain at one cell: every candidate already carries the pair of the cells it feeds."""
    stp = 0 if free_row else ext
    w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), (zl["zs"][0], zl["zs"][1] + 1))      # an opening
    if not free_row and ext > 0 and 0 >= w[0]:
        w = (0, 1, (0, 1))                                  # the floor of this very cell: a stop; the run begins right of it
    if first:                                               # the carry: out of a stop the run begins here
        w = _merge((feed["b"] + stp, 1, (feed["bs"][0], feed["bs"][1] + (feed["b"] <= 0))), w)
    if run is not None:
        w = _merge((run[0] + stp, run[1], run[2]), w)
    return w


def kernel_model(osc, a: bytes, b: bytes, strip_cols: int = 1 << 30, pay=None):
    """The five values the way the kernel finds them, payloads as (gap_runs_a, gap_runs_b)."""
    la, lb = len(a), len(b)
    W_ = la + 1
    M, A, B = SP._matrices(osc, a, b)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, no_gaps_b = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_b)
    D_ = [STOP] * W_                                                    # row 0
    V = list(D_)
    Ap, Yv, Xv = [0] * W_, [0] * W_, [0] * W_                           # the sweep's own row 0: all 0
    col_best = [0] * W_
    col_info = [None] * W_

    for y in range(1, lb + 1):
        r = y * W_
        free_row, forced = no_end and y == lb, no_gaps_b and y != lb
        nD, nV = [STOP] + [None] * la, [STOP] + [None] * la
        nAp, nYv, nXv = [0] * W_, [0] * W_, [0] * W_
        feed = dict(z=0, b=0, from_a=False, zs=STOP, bs=STOP)          # the border column
        for i0 in range(0, max(la, 1), strip_cols):
            hi = min(la, i0 + strip_cols)
            run, zl, out = None, feed, None
            for x in range(i0 + 1, hi + 1):
                m, av, bv = M[r + x], A[r + x], B[r + x]
                ms = D_[x - 1] if m > 0 else STOP                       # the match state adds nothing
                a_free = no_end and x == la
                as_ = _gap_a_state(av, D_[x] if a_free else V[x], a_free, Ap[x], Yv[x], Xv[x], open1, ext, osc.gap_open)
                if forced:
                    bs = STOP
                else:
                    run = _gap_b_candidate(zl, feed, x == i0 + 1, run, free_row, open1, ext)
                    assert max(run[0], 0) == bv, (x, y, run, bv)
                    bs = run[2] if bv > 0 else STOP
                if pay is not None:                                     # the definition, state by state
                    for st, got in ((MATCH, ms), (GAP_A, as_), (GAP_B, bs)):
                        assert got == pay[st][r + x], (st, x, y, got, pay[st][r + x])
                from_a = av >= m
                zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
                mb = max(m, bv)
                low = bs if bv >= m else ms
                nD[x] = as_ if av >= mb else low
                nV[x] = as_ if av + ext >= mb + open1 else low
                nAp[x], nYv[x], nXv[x] = av, mb, max(av, mb)
                if m > col_best[x]:
                    col_best[x], col_info[x] = m, ((x, y), ms)
                out = dict(z=zl["z"], b=bv, from_a=from_a, zs=zl["zs"], bs=bs)
            if hi < la:                                                 # what this strip hands the next one: raw
                feed = out
                zwins = (feed["z"] >= feed["b"]) if feed["from_a"] else (feed["z"] > feed["b"])
                assert nD[hi] == (feed["zs"] if zwins else feed["bs"]), (hi, y)
        D_, V, Ap, Yv, Xv = nD, nV, nAp, nYv, nXv
    best, best_at, words = 0, None, None
    for x in range(1, W_):
        if col_best[x] > best:
            best, (best_at, words) = col_best[x], col_info[x]
    return _result(best, best_at, words)


def frame_model(osc, a: bytes, b: bytes, lo: int, hi: int, F: int = 8, pay=None):
    """The five values the way the banded kernel finds them with a frame of F positions.  pay: the definition's pairs over the
    banded matrices (forward with mats) -- every band cell's three states are then compared with them.  The values above a cell
    (gap_a above, max(M, B) above) are the banded matrices', where a cell outside the band holds 0: what the shell's rule 2
    writes into the frame."""
    la, lb = len(a), len(b)
    band = BS.clip(la, lb, lo, hi)
    if band is None or la == 0:
        return ZEROS
    d_lo, d_hi = band
    assert d_hi - d_lo + 1 <= F
    W_ = la + 1
    M, A, B = BSP.banded_mats(osc, a, b, lo, hi)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, no_gaps_b = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_b)
    first = 1 - d_hi if d_hi < 0 else 1
    rows = min(lb, la - d_lo)

    D = [STOP] * F                                          # the zeros of row first - 1: what start_strip wrote
    V = list(D)
    bound_d = STOP
    bs, binfo = [0] * F, [None] * F
    ret = (0, None, None)                                   # best value, (column, row), the two words of the retired columns

    fc = max(1, d_lo)
    for j in range(first, rows + 1):
        fc = max(1, j + d_lo)
        if j + d_lo >= 2:                                   # rule 1: the frame moves
            bound_d = D[0]
            D, V = D[1:] + [POISON], V[1:] + [POISON]
            if bs[0] > ret[0]:                              # rule 3: column fc - 1 retires; a tie stays with the retired
                ret = (bs[0], (fc - 1, binfo[0][0]), binfo[0][1])
            bs, binfo = bs[1:] + [0], binfo[1:] + [None]
        ge = j + d_hi - fc
        assert 0 <= ge < F
        V[ge] = STOP                                        # rule 2: the cell above the right edge
        n_row = min(la, j + d_hi) - fc + 1
        feed = dict(z=0, b=0, from_a=False, zs=STOP, bs=STOP)
        dprev, bound_d = bound_d, STOP                      # the feed becomes the up-left of position 0 on the next row
        nD, nV = [POISON] * F, [POISON] * F                 # rule 4: positions without a band cell
        free_row, forced = no_end and j == lb, no_gaps_b and j != lb
        run, zl = None, feed
        for g in range(max(0, n_row)):
            x = fc + g
            at = j * W_ + x
            up = at - W_
            m, av, bv = int(M[at]), int(A[at]), int(B[at])
            ap, yv = int(A[up]), max(int(M[up]), int(B[up]))
            if j == first:
                assert ap == 0 and yv == 0
            ms = dprev if m > 0 else STOP
            a_free = no_end and x == la
            as_ = _gap_a_state(av, D[g] if a_free else V[g], a_free, ap, yv, max(ap, yv), open1, ext, osc.gap_open)
            if forced:
                bsp = STOP
            else:
                run = _gap_b_candidate(zl, feed, g == 0, run, free_row, open1, ext)
                assert max(run[0], 0) == bv, (x, j, run, bv)
                bsp = run[2] if bv > 0 else STOP
            assert POISON not in (ms, as_, bsp), (x, j)     # a band cell never reads a position without one
            if pay is not None:
                for st, got in ((MATCH, ms), (GAP_A, as_), (GAP_B, bsp)):
                    assert got == pay[st][at], (st, x, j, got, pay[st][at])
            from_a = av >= m
            zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
            mb = max(m, bv)
            low = bsp if bv >= m else ms
            nD[g] = as_ if av >= mb else low
            nV[g] = as_ if av + ext >= mb + open1 else low
            if m > bs[g]:
                bs[g], binfo[g] = m, (j, ms)
            dprev = D[g]
        D, V = nD, nV
    best, at, words = 0, None, None
    for g in range(F):                                      # the live columns ascending
        if bs[g] > best:
            best, at, words = bs[g], (fc + g, binfo[g][0]), binfo[g][1]
    if ret[0] >= best and ret[0] > 0:                       # a tie goes to the retired, lower column
        best, at, words = ret
    return _result(best, at, words)


# ----------------------------------------------------------------------------------------------------------- pairs ---
def _rand(rng, n, alpha):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


def gap_rich_pairs(seed: int, n: int, alpha: bytes = b"ACGT", length: int = 45):
    """(a, b): b is a with one block of 1 .. 3 letters deleted in the first half and one inserted in the second (odd pairs: the
    other way round), so a hit that spans both has a run in each string."""
    rng = W.Rng(seed)
    pairs = []
    for k in range(n):
        a = _rand(rng, length, alpha)
        d, i = (int(v) for v in rng.below(3, 2))
        at_d = length // 3 + int(rng.below(3, 1)[0])
        at_i = 2 * length // 3 + int(rng.below(3, 1)[0])
        b = a[:at_d] + a[at_d + d + 1:at_i] + _rand(rng, i + 1, alpha) + a[at_i:]
        pairs.append((b, a) if k % 2 else (a, b))
    return pairs


LONG = 66000                       # past SEQALIGN_SW_STATS_MAX_LEN = 65 535
BLOCK_INIT = [1, -3, -5, -1]       # a gap of 40 costs 45, each flank scores thousands: one hit, one run


def deleted_block(rng, n: int = LONG, at: int = 30000, block: int = 40):
    """(a, a without a[at:at + block]) over ACGT: under BLOCK_INIT the best hit is the whole of both with one run of `block`
    '-' in string b: end (n, n - block), runs (0, 1).  The GPU tests hold the call to the strings of the align calls besides."""
    a = bytes(b"ACGT"[i] for i in rng.below(4, n))
    return a, a[:at] + a[at + block:]
