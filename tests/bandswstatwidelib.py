"""Helpers of the wide banded SW statistics tests (seqalign_sw_stats_banded_wide).  Not a test module.

strip_model         the kernel's schedule (sa_band_frame.hpp) in pure Python over payloads IN PACKED
                    FORM (cell word, counts word; masked to 32 bits), values from bandswlib.fill: the strips of S columns and
                    their rows, the standing and the moving frame, the stop feed and the left strip's hand-off entry, the up-left
                    of a strip's first row, the reset of V above the right edge, the hand-off entries and which rows have one,
                    the retire, the end pick per strip (live columns, then the retired best first on a tie), the merge of the
                    left strip's best entry (left wins a tie) and the unpacking in the last strip of the run.  Strips run left
                    to right, each over all its rows: the order the pipeline's waits enforce per row.  Every frame position that
                    holds no band cell of the strip, every hand-off entry and every best entry that is never written carry
                    POISON, and the model asserts that no band cell and no merge reads one.  Modelled on bandstatlib.frame_model,
                    whose cell arithmetic this repeats;
band_kind           "empty", "left", "right" or "mid": where the clipped band lies relative to the main diagonal;
crosses_seam        whether a hit's letters have columns in more than one strip of S columns;
outside_left_of_seam   whether a hit starts outside the band in a strip left of the one it ends in;
long_band_pairs     pairs long enough for several strips at S = 7 with bands of up to 14 diagonals.
"""
from __future__ import annotations

import random

import bandlib as BL
import bandspanlib as BSP
import bandswlib as BS
import statlib as ST
import swstatlib as SS

ZEROS = SS.ZEROS
POISON = None
STANDING, MOVING = "standing", "moving"


def band_kind(la: int, lb: int, lo: int, hi: int) -> str:
    band = BS.clip(la, lb, lo, hi)
    if band is None:
        return "empty"
    return "left" if band[1] < 0 else "right" if band[0] > 0 else "mid"


def crosses_seam(seven, S: int) -> bool:
    """The hit's letters of seq_a are columns pos_a + 1 .. pos_a + len_a."""
    return seven[0] > 0 and seven[3] > 0 and seven[1] // S < (seven[1] + seven[3] - 1) // S


def outside_left_of_seam(seven, la: int, lb: int, lo: int, hi: int, S: int) -> bool:
    """The hit's stop cell (pos_a, pos_b) lies outside the band, in an inner column, and in a strip left of its end's."""
    return BSP.starts_outside(seven[:5], la, lb, lo, hi) and seven[1] >= 1 and (seven[1] - 1) // S < (seven[1] + seven[3] - 1) // S


def strip_model(osc, a: bytes, b: bytes, lo: int, hi: int, S: int, mats=None):
    """((score, pos_a, pos_b, len_a, len_b, matches, mismatches), coverage) the way band_payload_strips_kernel finds them with
    strips of S columns.  coverage: strips, busy (strips with rows), late_start (strips with jf > 1), both_phases (strips that
    stand and then move), entries (hand-off entries written), stop_feeds (rows fed by a stop), tie_left (merges in which the
    left strip's best equals mine), tie_retired (end picks in which the retired best equals the live one)."""
    la, lb = len(a), len(b)
    assert la <= SS.MAX_LEN and lb <= SS.MAX_LEN
    F = S
    cover = dict(strips=max(1, -(-la // F)), busy=0, late_start=0, both_phases=0, entries=0, stop_feeds=0, tie_left=0, tie_retired=0)
    band = BS.clip(la, lb, lo, hi)
    d_lo, d_hi = band if band is not None else (la, la)      # an empty band: the one diagonal len_a, which has no inner cell
    width = d_hi - d_lo + 1
    W_ = la + 1
    M, A, B = mats or ((None,) * 3 if band is None or not la or not lb else BSP.banded_mats(osc, a, b, lo, hi))
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, no_gaps_b = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_b)
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)

    def stop(x, y):                                          # a stop that has counted nothing
        return (SS.pack_cell(x, y), 0)

    def merge(l, r):
        return l if l[0] >= r[0] + r[1] else r

    def boundary(feed):                                      # row()'s boundary rule: A >= B > M via from_a
        zwins = (feed["z"] >= feed["b"]) if feed["from_a"] else (feed["z"] > feed["b"])
        return feed["zs"] if zwins else feed["bs"]

    def in_band(x, y):
        return 1 <= x <= la and 1 <= y <= lb and d_lo <= x - y <= d_hi

    result = None
    hand_in, best_in = None, POISON
    for s in range(cover["strips"]):
        c0 = s * F
        cend = min(la, c0 + F)
        jf, jl = max(1, c0 + 1 - d_hi), (min(lb, cend - d_lo) if la else 0)
        jl_left = min(lb, c0 - d_lo)
        left_rows = s > 0 and jl_left >= 1
        right_rows = lb >= 1 and c0 + F < la and c0 + F + 1 <= lb + d_hi
        hand_out, best_out = [POISON] * width, POISON
        if jf > jl:                                          # no band cell in my columns
            if s == 0 and (la == 0 or lb == 0 or max(1, 1 + d_lo) > min(la, lb + d_hi)):
                assert result is None
                result = ZEROS
            hand_in, best_in = hand_out, best_out
            continue
        cover["busy"] += 1
        cover["late_start"] += jf > 1
        fc0 = max(c0 + 1, d_lo)                              # the frame of the row before my first
        assert jf == 1 or fc0 == c0 + 1

        def first_stop(x):                                   # row jf - 1: a border row or outside the band in all my columns
            assert not in_band(x, jf - 1)
            return stop(x, jf - 1) if x <= cend else POISON   # (past the strip's end or len_a the word may be garbage)

        D = [first_stop(fc0 + g) for g in range(F)]
        V = list(D)
        bound_d = stop(fc0 - 1, jf - 1)
        assert fc0 - 1 <= la
        if jf > 1 and s > 0:                                 # cell (c0, jf - 1), on the band's right edge: hand-off entry 0
            assert left_rows and hand_in[0] is not POISON, ("the up-left of a strip's first row", s)
            e0 = hand_in[0]
            at = (jf - 1) * W_ + c0
            assert (e0["z"], e0["b"]) == (max(M[at], A[at]), B[at])
            bound_d = boundary(e0)
        bs, binfo = [0] * F, [None] * F
        ret = (0, None, None)
        phases = set()
        fc = fc0
        for j in range(jf, jl + 1):
            r = j * W_
            jd = j + d_lo
            fc = max(c0 + 1, jd)
            moving = jd >= c0 + 2
            phases.add(MOVING if moving else STANDING)
            if moving:                                       # rule 1: the frame moves; a column past the strip's end enters
                bound_d = D[0]
                D, V = D[1:] + [POISON], V[1:] + [POISON]
                if bs[0] > ret[0]:                           # column fc - 1 retires; a tie stays with the retired
                    ret = (bs[0], (fc - 1, binfo[0][0]), binfo[0][1])
                bs, binfo = bs[1:] + [0], binfo[1:] + [None]
            ge = j + d_hi - fc
            assert ge >= 0
            if ge < F:                                       # rule 2: the cell above the right edge
                assert not in_band(j + d_hi, j - 1)
                V[ge] = stop(j + d_hi, j - 1) if j + d_hi <= cend else POISON
            e = j - (c0 - d_hi)                              # the cell left of the frame
            if s > 0 and 0 <= e < width:
                assert left_rows and j <= jl_left and hand_in[e] is not POISON, ("a hand-off entry that was never written", s, j, e)
                feed = hand_in[e]
                assert not moving and in_band(c0, j) and (feed["z"], feed["b"]) == (max(M[r + c0], A[r + c0]), B[r + c0]), (s, j)
            else:
                assert not in_band(fc - 1, j) and fc - 1 <= la, (s, j)
                left = stop(fc - 1, j)
                feed = dict(z=0, b=0, from_a=False, zs=left, bs=left)
                cover["stop_feeds"] += 1
            dprev, bound_d = bound_d, boundary(feed)         # the feed becomes the up-left of position 0 on the next row
            n_row = min(cend, j + d_hi) - fc + 1
            assert 1 <= n_row <= F, (s, j, n_row)
            nD, nV = [POISON] * F, [POISON] * F              # positions without a band cell of this strip
            free_row, forced = no_end and j == lb, no_gaps_b and j != lb
            run, zl = None, feed
            cells = [None] * F
            for g in range(n_row):
                x = fc + g
                assert in_band(x, j)
                at = r + x
                m, av, bv = M[at], A[at], B[at]
                here = stop(x, j)
                assert dprev is not POISON, ("the up-left", s, x, j)
                ms = (dprev[0], SS.count_step(dprev[1], fa[x - 1] == fb[j - 1])) if m > 0 else here
                a_free = no_end and x == la
                as_ = ((D[g] if a_free else V[g]) if av > 0 else here)
                if forced:
                    bsp = here
                else:
                    step = 0 if free_row else ext
                    w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"])
                    if not free_row and ext > 0 and 0 >= w[0]:
                        w = (0, 1, here)                     # the floor of this very cell
                    if g == 0:
                        w = merge((feed["b"] + step, 1, feed["bs"]), w)
                    if run is not None:
                        w = merge((run[0] + step, run[1], run[2]), w)
                    run = w
                    assert max(run[0], 0) == bv, (s, x, j, run, bv)
                    bsp = run[2] if bv > 0 else here
                assert POISON not in (ms, as_, bsp), (s, x, j)      # a band cell never reads a position without one
                from_a = av >= m
                zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
                cells[g] = dict(z=zl["z"], b=bv, from_a=from_a, zs=zl["zs"], bs=bsp)
                mb = max(m, bv)
                low = bsp if bv >= m else ms
                nD[g] = as_ if av >= mb else low
                nV[g] = as_ if av + ext >= mb + open1 else low
                if m > bs[g]:
                    bs[g], binfo[g] = m, (j, ms)
                dprev = D[g]
            D, V = nD, nV
            if right_rows and j + d_hi >= c0 + F:            # my last column is in the band on this row: entry [row - e_out0]
                out = cells[c0 + F - fc]
                assert out is not None, ("the strip's last column holds no cell", s, j)
                eo = j - (c0 + F - d_hi)
                assert 0 <= eo < width and hand_out[eo] is POISON
                hand_out[eo] = out
                cover["entries"] += 1
        if phases == {STANDING, MOVING}:
            cover["both_phases"] += 1
        best, at, words = 0, None, None
        for g in range(F):                                   # the live columns of the last row's frame, ascending
            if bs[g] > best:
                best, at, words = bs[g], (fc + g, binfo[g][0]), binfo[g][1]
        if ret[0] >= best and ret[0] > 0:                    # a tie goes to the retired, lower column
            cover["tie_retired"] += ret[0] == best and at is not None
            best, at, words = ret
        if left_rows:                                        # the best of the strips to my left; a tie goes to them
            assert best_in is not POISON, ("the left strip's best entry was never written", s)
            if best_in[0] >= best and best_in[0] > 0:
                cover["tie_left"] += best_in[0] == best
                best, at, words = best_in
        if right_rows:
            best_out = (best, at, words) if best > 0 else (0, (0, 0), (0, 0))
        else:                                                # the last strip of the run
            assert result is None
            if best <= 0:
                result = ZEROS
            else:
                u64 = (words[0] << 32) | words[1]            # reduce_best's one word, and the write's unpacking
                (x0, y0), m_, mm = SS.unpacked((u64 >> 32, u64 & SS.MASK))
                result = (best, x0, y0, at[0] - x0, at[1] - y0, m_, mm)
        hand_in, best_in = hand_out, best_out
    assert result is not None
    return result, cover


def long_band_pairs(seed: int, n: int, alpha: bytes, lo_len: int = 15, hi_len: int = 40, max_width: int = 14):
    """[(a, b, lo, hi)]: n pairs of lo_len .. hi_len letters, every second a mutated relative; lo in [-len_b - 3, len_a + 3],
    width 1 .. max_width: bands left of, right of and across the main diagonal, and some empty after clipping."""
    rng = random.Random(seed)

    def rand_seq():
        return bytes(rng.choice(alpha) for _ in range(rng.randrange(lo_len, hi_len + 1)))

    out = []
    for k in range(n):
        a = rand_seq()
        b = BL.mutate(rng, a, 0.2, alpha) if k % 2 else rand_seq()
        lo = rng.randrange(-len(b) - 3, len(a) + 4)
        out.append((a, b, lo, lo + rng.randrange(max_width)))
    return out
