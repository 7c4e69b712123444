"""CPU tier: the argument behind the wide banded calls' kernel, on the Python definitions alone (no device).

strip_fill() restates band_strips_kernel's schedule in numpy for any strip width S: strip s owns columns s S + 1 .. (s + 1) S
and sweeps only the rows on which one of them is in the band, in a frame of S positions whose first column is
max(c0 + 1, j + d_lo) -- standing until the band's left edge enters the strip, then moving one column per row.  A strip
never reads another strip's cells: what it knows of its left neighbour is the hand-off column, per row max(M, A) and B of
that strip's last column where the cell is in the band; past the hand-off's rows, and once the frame has moved, the feed
is the floor.  The one position above the band's right edge gets the floor before every row.  Every other frame position
that holds no band cell of the strip -- right of the band, past the strip's end, past len_a -- is POISONED with a huge
value after every row and on entry, so a band cell that read one would be wrong: the test shows that none does.

It must reproduce bandlib.fill / bandswlib.fill on every cell, the NW end value, and the SW best cell in hit order (each
strip merges the best of the strips on its left; a tie stays left), for S in {1, 2, 3, 7, 64}, over the 32 flag
combinations, gap_open > 0 and gap_extend > 0 included."""
import itertools
import random

import numpy as np
import pytest

import bandlib as BL
import bandswlib as BS
import orclib as O

POISON = 1 << 40
# match, mismatch, gap_open, gap_extend: plain, affine, gap_open > 0, gap_extend > 0
SCORINGS = [(1, -1, -2, -1), (2, -3, -4, -1), (5, -4, 3, -4), (3, -2, -5, 1)]
COMBOS = list(itertools.product([0, 1], repeat=5))


def strip_fill(sc, a: bytes, b: bytes, d_lo: int, d_hi: int, S: int, sw: bool):
    """(M, A, B as bandlib.fill returns them, NW end value or SW best cell) by the strip schedule."""
    la, lb = len(a), len(b)
    go, ge = sc.gap_open + sc.gap_extend, sc.gap_extend
    mn = 0 if sw else BL.INT_MIN + abs(sc.min_penalty)
    if sw:
        M = np.zeros((lb + 1, la + 1), np.int64)
        A, B = M.copy(), M.copy()
    else:
        M, A, B = BL._borders(sc, la, lb, d_lo, d_hi, mn)      # strip 0 writes the band's border cells
    score, same, known = BL.scoring_table(sc, a, b)[2]
    ca, cb = np.frombuffer(a, np.uint8).astype(np.intp), np.frombuffer(b, np.uint8).astype(np.intp)
    no_mm, no_end, no_ga, no_gb = bool(sc.no_mismatches), bool(sc.no_end_gap_penalty), bool(sc.no_gaps_in_a), bool(sc.no_gaps_in_b)

    def edge_gap(k):
        return 0 if (sw or sc.no_start_gap_penalty) else sc.gap_open + k * ge

    strips = max(1, -(-la // S))
    hand = [dict() for _ in range(strips)]          # strip -> {row: (max(M, A), B) of its last column}, band cells only
    best_chain = None                               # (score, column, row) of the strips so far that had rows
    end_value = None
    for s in range(strips):
        c0 = s * S
        cend = min(la, c0 + S)
        jf, jl = max(1, c0 + 1 - d_hi), (min(lb, cend - d_lo) if la else 0)
        if jf > jl:
            if not sw and la and cend == la:       # NW, len_b = 0: the end value is a border cell
                end_value = max(mn, edge_gap(la))
            continue
        # the frame of the row before my first, on column max(c0 + 1, d_lo)
        fc = max(c0 + 1, d_lo)
        pM = np.full(S, POISON, np.int64)
        pA, pB = pM.copy(), pM.copy()
        if jf == 1:
            for g in range(S):                      # row 0: border cells, inside the band only
                col = fc + g
                if col <= min(la, d_hi):
                    pM[g], pA[g], pB[g] = mn, mn, max(mn, edge_gap(col))
            bound = 0 if c0 == 0 else max(mn, edge_gap(c0))
            if fc > c0 + 1:
                bound = None                        # the frame moves on row 1: taken from the frame itself
        else:
            bound = mn if s == 0 else max(hand[s - 1][jf - 1])   # (c0, jf - 1): on the band's right edge
        bs = np.zeros(S, np.int64)                  # SW: best per frame position, its first row; the retired best
        br = np.zeros(S, np.int64)
        ret = (0, 0, 0)
        for j in range(jf, jl + 1):
            if j + d_lo >= c0 + 2:                  # the frame moves
                bound = max(pM[0], pA[0], pB[0])
                assert bound < POISON
                if bs[0] > ret[0]:
                    ret = (int(bs[0]), fc, int(br[0]))
                for arr, enters in ((pM, POISON), (pA, POISON), (pB, POISON), (bs, 0), (br, 0)):
                    arr[:-1] = arr[1:]
                    arr[-1] = enters
                fc += 1
            assert fc == max(c0 + 1, j + d_lo)
            ge_pos = j + d_hi - fc                  # above the band's right edge: the floor
            if ge_pos < S:
                pM[ge_pos] = pA[ge_pos] = pB[ge_pos] = mn
            n = min(cend, j + d_hi) - fc + 1
            assert 1 <= n <= S
            # the cell left of the frame
            if j + d_lo <= c0 + 1 and s == 0:
                feed = (max(mn, edge_gap(j)), mn) if (not sw and j <= -d_lo) else (mn, mn)
            elif j + d_lo <= c0 + 1 and c0 - d_hi <= j <= c0 - d_lo:
                feed = hand[s - 1][j]
            else:
                feed = (mn, mn)
            x, y = ca[fc - 1:fc - 1 + n], cb[j - 1]
            up3 = np.maximum(np.maximum(pM[:n], pA[:n]), pB[:n])
            diag = np.concatenate(([bound], up3[:n - 1]))
            m = np.maximum(diag + score[y, x], mn)
            if no_mm:
                m = np.where(same[y, x], m, mn)
            m = np.where(known[y, x], m, mn)
            Mu, Au, Bu = pM[:n], pA[:n], pB[:n]
            if no_ga:
                av = np.full(n, mn, np.int64)
            else:
                av = np.maximum(np.maximum(np.maximum(Mu, Bu) + go, Au + ge), mn)
            if fc + n - 1 == la:
                if no_end:
                    av[-1] = max(Mu[-1], Au[-1], Bu[-1])
                elif no_ga:
                    av[-1] = max(Mu[-1] + go, Au[-1] + ge, Bu[-1] + go, mn)
            if j == lb and no_end:
                o, e = 0, 0
            elif (not no_gb) or j == lb:
                o, e = go, ge
            else:
                o = None
            if o is None:
                bv = np.full(n, mn, np.int64)
            else:
                t = np.arange(n)
                z = np.concatenate(([feed[0]], np.maximum(m, av)[:n - 1]))
                cand = np.maximum(z + o, mn) - t * e
                cand[0] = max(cand[0], feed[1] + e)
                bv = np.maximum.accumulate(cand) + t * e
            assert max(m.max(), av.max(), bv.max()) < POISON // 2, "a band cell read a cell that is none of its strip's"
            M[j, fc:fc + n], A[j, fc:fc + n], B[j, fc:fc + n] = m, av, bv
            pM[:], pA[:], pB[:] = POISON, POISON, POISON
            pM[:n], pA[:n], pB[:n] = m, av, bv
            bound = max(feed)
            up = m > bs[:n]
            br[:n] = np.where(up, j, br[:n])
            bs[:n] = np.where(up, m, bs[:n])
            if c0 + S < la and j + d_hi >= c0 + S:   # my last column is in the band: hand it on
                g = c0 + S - fc
                hand[s][j] = (int(max(m[g], av[g])), int(bv[g]))
        if sw:
            mine = ret
            for g in range(S):
                if bs[g] > mine[0]:
                    mine = (int(bs[g]), fc + g, int(br[g]))
            if best_chain is not None and best_chain[0] >= mine[0] and best_chain[0] > 0:
                mine = best_chain                   # a tie stays with the lower columns
            best_chain = mine
        elif cend == la:
            g = la - fc
            end_value = int(max(pM[g], pA[g], pB[g]))
    if sw:
        result = best_chain if best_chain and best_chain[0] > 0 else (0, 0, 0)
    else:
        result = (0 if lb == 0 else max(mn, edge_gap(lb))) if la == 0 else end_value
    return M.astype(np.int32).ravel(), A.astype(np.int32).ravel(), B.astype(np.int32).ravel(), result


def _pair(rng, max_len):
    la = rng.randrange(0, max_len + 1)
    a = bytes(rng.choice(b"ACGT") for _ in range(la))
    if rng.random() < 0.6:
        b = BL.mutate(rng, a, 0.2)[:max_len]
    else:
        b = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, max_len + 1)))
    return a, b


# the strip width, and the longest sequence it is run on (narrow strips make many sweeps)
SIZES = [(1, 30), (2, 50), (3, 60), (7, 110), (64, 150)]


@pytest.mark.parametrize("S,max_len", SIZES)
def test_strip_schedule_reproduces_banded_nw(S, max_len):
    rng = random.Random(1500 + S)
    for trial in range(128):          # every flag combination meets each of the four scorings
        flags = COMBOS[trial % 32]
        sc = O.build_scoring({"init": [*SCORINGS[(trial // 32 + trial) % 4], *flags, 0]})
        a, b = _pair(rng, max_len)
        la, lb = len(a), len(b)
        w = rng.choice([0, 1, 2, rng.randrange(0, 12), rng.randrange(0, max_len), 2 * max_len])
        d_lo, d_hi = BL.band_of(la, lb, w)
        want = BL.fill(sc, a, b, (d_lo, d_hi))
        M, A, B, end = strip_fill(sc, a, b, d_lo, d_hi, S, sw=False)
        assert np.array_equal(M, want[0]) and np.array_equal(A, want[1]) and np.array_equal(B, want[2]), (S, trial, flags, la, lb, w)
        assert end == BL.end_value(*want), (S, trial, flags, la, lb, w)


@pytest.mark.parametrize("S,max_len", SIZES)
def test_strip_schedule_reproduces_banded_sw(S, max_len):
    rng = random.Random(2500 + S)
    n_hit = 0
    for trial in range(128):          # every flag combination meets each of the four scorings
        flags = COMBOS[trial % 32]
        sc = O.build_scoring({"init": [*SCORINGS[(trial // 32 + trial) % 4], *flags, 0]})
        a, b = _pair(rng, max_len)
        la, lb = len(a), len(b)
        lo = rng.randrange(-max_len - 10, max_len + 10)
        hi = lo + rng.choice([0, 1, rng.randrange(0, 12), rng.randrange(0, 2 * max_len)])
        if trial % 8 == 0:
            lo, hi = -lb, la                                  # the whole matrix
        want = BS.fill(sc, a, b, (lo, hi))
        band = BS.clip(la, lb, lo, hi)
        if band is None:
            band = (la, la)                                   # what the kernels get for an empty band: no inner cell
        M, A, B, best = strip_fill(sc, a, b, band[0], band[1], S, sw=True)
        assert np.array_equal(M, want[0]) and np.array_equal(A, want[1]) and np.array_equal(B, want[2]), (S, trial, flags, la, lb, lo, hi)
        assert best == BS.best_cell(want[0], la), (S, trial, flags, la, lb, lo, hi)
        n_hit += best[0] > 0
    assert n_hit >= 16, n_hit


def test_best_cell_ties_across_strips():
    """A unit repeated across strips ties with itself: the lowest column, then the lowest row, wins whatever S."""
    sc = O.build_scoring({"init": [2, -3, -4, -1, 0, 0, 0, 0, 0, 0]})
    unit = bytes(random.Random(5).choice(b"ACGT") for _ in range(20))
    for a, b in ((unit * 5, unit), (unit, unit * 5)):
        la, lb = len(a), len(b)
        for lo, hi in ((-lb, la), (25, la), (-lb, 30), (-45, -5)):
            want = BS.fill(sc, a, b, (lo, hi))
            band = BS.clip(la, lb, lo, hi) or (la, la)
            for S in (1, 7, 64):
                M, _, _, best = strip_fill(sc, a, b, band[0], band[1], S, sw=True)
                assert np.array_equal(M, want[0]) and best == BS.best_cell(want[0], la), (la, lb, lo, hi, S)
