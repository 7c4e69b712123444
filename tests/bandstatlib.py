"""Helpers of the banded SW statistics tests (seqalign_sw_stats_banded).  Not a test module.

want                what the call must return for one pair: the seven values of the oracle's first hit over the banded matrices
                    (bandswlib.expected, min_score = 1) with the counted columns of its strings (swstatlib.hit_fields), zeros
                    when there is none;
frame_model         bandspanlib.frame_model with counts beside the stop cell, IN PACKED FORM: the kernel's frame bookkeeping
                    (sa_band_frame.hpp, sa_band_stats.hip) -- positions, the shift, the edge cell's feed, the
                    feed left of the frame, the retire and the end pick -- over payloads (cell word, counts word) masked to 32
                    bits.  Values come from bandswlib.fill.  A position that holds no band cell carries POISON, so a band cell
                    that read one would show it;
counts_reversed_differ   whether a pair's COUNTS inside a band change under the reversed priority M > B > A;
tie_batch, tie_counts    the tie-dense batches of the GPU tier and, per batch and band, how many pairs are tie-sensitive in
                    their counts (on the oracle's banded matrices alone).
"""
from __future__ import annotations

import bandspanlib as BSP
import bandswlib as BS
import spanlib as SP
import statlib as ST
import swstatlib as SS

ZEROS = SS.ZEROS
POISON = None


def want(osc, a: bytes, b: bytes, lo: int, hi: int):
    """((score, end_a, end_b) of the banded score call, the seven values of the banded statistics call)."""
    cell, hit = BS.expected(osc, a, b, lo, hi, 1)
    return cell, SS.hit_fields(osc, [hit] if hit else [])


def got_stats(res):
    return SS.got_sw_stats(res)


def frame_model(osc, a: bytes, b: bytes, lo: int, hi: int, F: int = 8):
    """(score, pos_a, pos_b, len_a, len_b, matches, mismatches) the way band_sw_stats_rows_kernel finds them with a frame of F
    positions."""
    la, lb = len(a), len(b)
    assert la <= SS.MAX_LEN and lb <= SS.MAX_LEN
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
    c0 = max(1, d_lo)                                       # the frame's first column before the first row

    def stop(x, y):                                         # a stop that has counted nothing
        return (SS.pack_cell(x, y), 0)

    D = [stop(c0 + g, first - 1) for g in range(F)]         # the zeros of row first - 1
    V = list(D)
    bound_d = stop(c0 - 1, first - 1)
    bs, binfo = [0] * F, [None] * F
    ret = (0, None, None)                                   # best value, (column, row), the two words of the retired columns

    def merge(l, r):
        return l if l[0] >= r[0] + r[1] else r

    fc = c0
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
        V[ge] = stop(j + d_hi, j - 1)                       # rule 2: the cell above the right edge
        n_row = min(la, j + d_hi) - fc + 1
        left = stop(fc - 1, j)
        feed = dict(z=0, b=0, from_a=False, zs=left, bs=left)
        dprev, bound_d = bound_d, left                      # the feed becomes the up-left of position 0 on the next row
        nD, nV = [POISON] * F, [POISON] * F                 # rule 4: positions without a band cell
        free_row, forced = no_end and j == lb, no_gaps_b and j != lb
        run, zl = None, feed
        for g in range(max(0, n_row)):
            x = fc + g
            at = j * W_ + x
            m, av, bv = M[at], A[at], B[at]
            here = stop(x, j)
            ms = (dprev[0], SS.count_step(dprev[1], fa[x - 1] == fb[j - 1])) if m > 0 else here
            a_free = no_end and x == la
            as_ = ((D[g] if a_free else V[g]) if av > 0 else here)
            if forced:
                bsp = here
            else:
                step = 0 if free_row else ext
                w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"])
                if not free_row and ext > 0 and 0 >= w[0]:
                    w = (0, 1, here)                        # the floor of this very cell
                if g == 0:
                    w = merge((feed["b"] + step, 1, feed["bs"]), w)
                if run is not None:
                    w = merge((run[0] + step, run[1], run[2]), w)
                run = w
                assert max(run[0], 0) == bv, (x, j, run, bv)
                bsp = run[2] if bv > 0 else here
            assert POISON not in (ms, as_, bsp), (x, j)     # a band cell never reads a position without one
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
    if best <= 0:
        return ZEROS
    u64 = (words[0] << 32) | words[1]                       # reduce_best's one word, and the write's unpacking
    (x0, y0), m, mm = SS.unpacked((u64 >> 32, u64 & SS.MASK))
    return (best, x0, y0, at[0] - x0, at[1] - y0, m, mm)


def counts_reversed_differ(osc, a: bytes, b: bytes, lo: int, hi: int) -> bool:
    """Whether the pair's banded (matches, mismatches) change when the predecessor priority is reversed to M > B > A.  A change
    of the span alone does not count."""
    M, A, B = BS.fill(osc, a, b, (lo, hi))
    best = SP.best_cell_np(M, len(a))
    if best[0] <= 0:
        return False
    mats = (M, A, B)
    return SS.walk(osc, a, b, SS.WALKER, mats, best)[5:] != SS.walk(osc, a, b, SS.REVERSED, mats, best)[5:]


TIE_WIDTHS = BSP.TIE_WIDTHS
TIE_BANDS = BSP.TIE_BANDS
# The batches are bandspanlib.tie_batch's (spanlib.tie_pairs' first 40, or 80 where bandspanlib.TIE_N says so).  Where none of
# those changes its COUNTS inside a band under the reversed priority, the batch is lengthened from the same generator until
# one does; nothing is taken out.  test_sw_stats_banded_argument_cpu.py asserts the condition for every entry.
TIE_N = dict(BSP.TIE_N)


def tie_batch(name: str, width: int):
    return SP.tie_pairs(name, width, n=TIE_N.get((name, width), 40))


def tie_counts(osc_of):
    """{(scoring name, width, band): pairs of tie_batch(name, width) whose counts are tie-sensitive inside the band}."""
    out = {}
    for name in SP.TIE_SCORINGS:
        osc = osc_of(name)
        for width in TIE_WIDTHS:
            pairs = tie_batch(name, width)
            for lo, hi in TIE_BANDS:
                out[name, width, (lo, hi)] = sum(counts_reversed_differ(osc, a, b, lo, hi) for a, b in pairs)
    return out
