"""Helpers of the SW identity-count tests (seqalign_sw_counts_batch / _banded / _banded_wide).  Not a test module.

want_counts         what the unbanded call must return per pair, from the oracle's first hit: (score, end_a, end_b, matches,
                    mismatches) -- swstatlib.want_sw_stats' seven with pos + len folded into the end;
counts_of           the same five from a seven-tuple of the sw_stats family;
got_counts          sw_counts' five arrays as a list of such tuples;
kernel_model        the sweep's own shape on the CPU (sa_sw_counts.hpp): swstatlib.kernel_model with the payload
                    of a state LITERALLY two unmasked Python ints (matches, mismatches) and no stop cell -- a stop is (0, 0)
                    wherever it is; strips hand on {max(M, A), B, whether A's, the two pairs}.  With pay = swstatlib.forward's
                    payloads every state of every cell is compared with the cnt half of the definition;
frame_model         bandstatlib.frame_model in the same form: the band frame's bookkeeping (sa_band_frame.hpp,
                    sa_band_counts.hip) over pairs of unmasked ints; a position without a band cell carries POISON;
self_pair, apart    the two constructed long pairs whose results hold by construction;
host_counts         (score, end_a, end_b, matches, mismatches) of a hit dict with its strings counted on the host.
"""
from __future__ import annotations

import bandspanlib as BSP
import bandswlib as BS
import spanlib as SP
import statlib as ST
import swstatlib as SS

MATCH, GAP_A, GAP_B = SS.MATCH, SS.GAP_A, SS.GAP_B
ZEROS = (0, 0, 0, 0, 0)
POISON = None
STOP = (0, 0)                      # a state that stops has counted nothing, wherever it stops


def counts_of(seven):
    """(score, end_a, end_b, matches, mismatches) of (score, pos_a, pos_b, len_a, len_b, matches, mismatches)."""
    s, pa, pb, la, lb, m, mm = (int(v) for v in seven)
    return (s, pa + la, pb + lb, m, mm)


def want_counts(osc, pairs):
    return [counts_of(w) for w in SS.want_sw_stats(osc, pairs)]


def got_counts(res):
    return [tuple(int(x[p]) for x in res) for p in range(len(res[0]))]


def host_counts(osc, hits):
    return counts_of(SS.hit_fields(osc, hits))


def step(pay, eq: bool):
    """A match state's own letters: one add to one of two full words.  No mask: the test asserts the values stay below 2^32."""
    return (pay[0] + 1, pay[1]) if eq else (pay[0], pay[1] + 1)


def _result(best, at, words):
    if best <= 0:
        return ZEROS
    u64 = (words[0] << 32) | words[1]                                   # reduce_best's one word, and the write's two halves
    assert 0 <= words[0] < 1 << 32 and 0 <= words[1] < 1 << 32
    return (best, at[0], at[1], u64 >> 32, u64 & SS.MASK)


def kernel_model(osc, a: bytes, b: bytes, strip_cols: int = 1 << 30, pay=None):
    """The five values the way the kernel finds them, payloads as (matches, mismatches)."""
    la, lb = len(a), len(b)
    W = la + 1
    M, A, B = SP._matrices(osc, a, b)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, no_gaps_b = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_b)
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)
    D_ = [STOP] * W                                                     # row 0
    V = list(D_)
    col_best = [0] * W
    col_info = [None] * W

    def merge(l, r):                       # l lies left of r: r wins a tie unless it is an opening from M (nm = 0)
        return l if l[0] >= r[0] + r[1] else r

    for y in range(1, lb + 1):
        r = y * W
        free_row, forced = no_end and y == lb, no_gaps_b and y != lb
        nD, nV = [STOP] + [None] * la, [STOP] + [None] * la
        feed = dict(z=0, b=0, from_a=False, zs=STOP, bs=STOP)          # the border column
        for i0 in range(0, max(la, 1), strip_cols):
            hi = min(la, i0 + strip_cols)
            run, zl, out = None, feed, None
            for x in range(i0 + 1, hi + 1):
                m, av, bv = M[r + x], A[r + x], B[r + x]
                ms = step(D_[x - 1], fa[x - 1] == fb[y - 1]) if m > 0 else STOP
                a_free = no_end and x == la
                as_ = ((D_[x] if a_free else V[x]) if av > 0 else STOP)
                if forced:
                    bs = STOP
                else:
                    stp = 0 if free_row else ext
                    w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"])
                    if not free_row and ext > 0 and 0 >= w[0]:
                        w = (0, 1, STOP)                                # the floor of this very cell
                    if x == i0 + 1:
                        w = merge((feed["b"] + stp, 1, feed["bs"]), w)
                    if run is not None:
                        w = merge((run[0] + stp, run[1], run[2]), w)
                    run = w
                    assert max(run[0], 0) == bv, (x, y, run, bv)
                    bs = run[2] if bv > 0 else STOP
                if pay is not None:                                     # the cnt half of the definition, state by state
                    for st, got in ((MATCH, ms), (GAP_A, as_), (GAP_B, bs)):
                        assert got == pay[st][r + x][1:], (st, x, y, got, pay[st][r + x])
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
    return _result(best, best_at, words)


def frame_model(osc, a: bytes, b: bytes, lo: int, hi: int, F: int = 8, pay=None):
    """(score, end_a, end_b, matches, mismatches) the way the banded kernel finds them with a frame of F positions.  pay: the
    definition's payloads over the banded matrices (swstatlib.forward with mats) -- every band cell's three states are then
    compared with its cnt half."""
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
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)
    first = 1 - d_hi if d_hi < 0 else 1
    rows = min(lb, la - d_lo)

    D = [STOP] * F                                          # the zeros of row first - 1: what start_strip wrote
    V = list(D)
    bound_d = STOP
    bs, binfo = [0] * F, [None] * F
    ret = (0, None, None)                                   # best value, (column, row), the two words of the retired columns

    def merge(l, r):
        return l if l[0] >= r[0] + r[1] else r

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
            m, av, bv = M[at], A[at], B[at]
            ms = step(dprev, fa[x - 1] == fb[j - 1]) if m > 0 else STOP
            a_free = no_end and x == la
            as_ = ((D[g] if a_free else V[g]) if av > 0 else STOP)
            if forced:
                bsp = STOP
            else:
                stp = 0 if free_row else ext
                w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"])
                if not free_row and ext > 0 and 0 >= w[0]:
                    w = (0, 1, STOP)                        # the floor of this very cell
                if g == 0:
                    w = merge((feed["b"] + stp, 1, feed["bs"]), w)
                if run is not None:
                    w = merge((run[0] + stp, run[1], run[2]), w)
                run = w
                assert max(run[0], 0) == bv, (x, j, run, bv)
                bsp = run[2] if bv > 0 else STOP
            assert POISON not in (ms, as_, bsp), (x, j)     # a band cell never reads a position without one
            if pay is not None:
                for st, got in ((MATCH, ms), (GAP_A, as_), (GAP_B, bsp)):
                    assert got == pay[st][at][1:], (st, x, j, got, pay[st][at])
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


# ---------------------------------------------------------------------------------- pairs that hold by construction ---
LONG = 66000                       # past SEQALIGN_SW_STATS_MAX_LEN = 65 535
SELF_INIT = [1, -2, -4, -1]        # a sequence against itself: the main diagonal, LONG matches
APART_INIT = [1, 1, -4, -1]        # mismatch scores +1: b"A" * n against b"C" * n is the main diagonal, LONG mismatches


def self_pair(rng, n: int = LONG):
    """(a, a) over ACGT without a repeat structure worth a gap: under SELF_INIT the only best hit is the whole diagonal, so the
    call wants (n, n, n, n, 0)."""
    a = bytes(b"ACGT"[i] for i in rng.below(4, n))
    return a, a


def apart_pair(n: int = LONG):
    """(A^n, C^n): under APART_INIT every diagonal step scores +1 and every gap loses, so the best cell is (n, n) with score n
    and the walk is n mismatches: (n, n, n, 0, n)."""
    return b"A" * n, b"C" * n
