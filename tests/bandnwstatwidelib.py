"""Helpers of the wide banded NW statistics tests (seqalign_nw_stats_banded_wide).  Not a test module.

strip_model         the kernel's schedule (sa_band_nw_stats_strips.hip) in pure Python over payloads (matches,
                    mismatches, mark), values from bandlib.fill: the strips of S columns and their rows, the standing and the
                    moving frame, the three feeds (the border column, the left strip's hand-off entry, nothing), the up-left of a
                    strip's first row, the reset of V AND D of the cell above the right edge, the hand-off entries and which rows
                    have one, the end pick in the last strip.  Strips run left to right, each over all its rows: the order the
                    pipeline's waits enforce per row.  Every frame position that holds no band cell of the strip and every
                    hand-off entry that is never written carry POISON, and the model asserts that no band cell reads one.
                    Modelled on bandnwstatlib.frame_model, whose cell arithmetic this repeats;
walk_crosses_seam   whether the counted part of an alignment (its cells with x > 0 and y > 0) lies in more than one strip;
long_pairs          pairs long enough for at least three strips at S = 7, len_a < len_b and len_a > len_b;
definition_cases    the GPU tier's scorings and pairs of the 32 flag combinations.
"""
from __future__ import annotations

import random

import bandlib as BL
import bandnwstatlib as BN
import statlib as ST

POISON = None
Z, MARK = (0, 0, False), (0, 0, True)
BORDER, HANDOFF, NOTHING = "border", "hand-off", "nothing"      # the three feeds of a standing frame
STANDING, MOVING = "standing", "moving"


def strip_model(osc, a: bytes, b: bytes, w: int, S: int, mats=None):
    """((score, matches, mismatches), whether the end state carries the mark, coverage) the way band_nw_stats_strips_kernel finds
    them with strips of S columns.  coverage: feeds0 (the feeds strip 0's rows took, MOVING for its rows of the moving phase),
    late_start (strips s > 0 with jf > 1), both_phases (strips s > 0 with standing and moving rows), marked / from_a (hand-off
    entries that carry the mark / an admitted gap_a's max(M, A)), entries, strips."""
    la, lb = len(a), len(b)
    W_ = la + 1
    d_lo, d_hi = BL.band_of(la, lb, w)
    width = d_hi - d_lo + 1
    M, A, B = mats or tuple(X.tolist() for X in BL.fill(osc, a, b, (d_lo, d_hi)))
    score = ST.end_pick(M, A, B, W_ * (lb + 1) - 1)[1]
    cover = dict(feeds0=set(), late_start=0, both_phases=0, marked=0, from_a=0, entries=0, strips=max(1, -(-la // S)))
    if la == 0:                                              # strip 0 writes the border cell and (0, 0)
        return (score, 0, 0), False, cover
    fl = ST.floor_of(osc)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, nga, ngb, no_mm = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_a), bool(osc.no_gaps_in_b), bool(osc.no_mismatches)
    look = ST.Lookup(osc)
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)
    F = S

    def merge(l, r):                                         # l lies left of r: r wins a tie only as an opening from A
        return l if l[0] >= r[0] + r[1] else r

    def boundary(feed, j):                                   # row()'s boundary rule: D of the feed cell, `forced` as on row j
        forced = ngb and j != lb
        zwins = forced or ((feed["z"] >= feed["b"]) if feed["from_a"] else (feed["z"] > feed["b"]))
        return feed["zs"] if zwins else feed["bs"]

    nothing = dict(z=fl, b=fl, from_a=False, zs=MARK, bs=MARK)
    result = None
    hand_in = None
    for s in range(cover["strips"]):
        c0 = s * F
        cend = min(la, c0 + F)
        jf, jl = max(1, c0 + 1 - d_hi), min(lb, cend - d_lo)
        right_rows = lb >= 1 and c0 + F < la and c0 + F + 1 <= lb + d_hi
        hand_out = [POISON] * width
        phases = set()
        if jf == 1:                                          # row 0: the border's band cells, columns c0 + 1 .. d_hi
            D = [Z if c0 + 1 + g <= min(la, d_hi) else POISON for g in range(F)]
            assert c0 <= d_hi
            bound_d = Z                                      # cell (c0, 0): on the border and in the band
        else:                                                # row jf - 1 has no band cell in my columns
            D = [POISON] * F
            cover["late_start"] += s > 0
            if s == 0:
                bound_d = MARK
            else:                                            # cell (c0, jf - 1), on the band's right edge: hand-off entry 0
                assert hand_in[0] is not POISON, ("the up-left of a strip's first row", s)
                e = hand_in[0]
                assert (e["z"], e["b"]) == (max(M[(jf - 1) * W_ + c0], A[(jf - 1) * W_ + c0]), B[(jf - 1) * W_ + c0])
                bound_d = boundary(e, jf - 1)
        V = list(D)
        for j in range(jf, jl + 1):
            r = j * W_
            jd = j + d_lo
            fc = max(c0 + 1, jd)
            moving = jd >= c0 + 2
            phases.add(MOVING if moving else STANDING)
            if moving:                                       # rule 1: the frame moves; a column past the strip's end enters
                bound_d = D[0]
                D, V = D[1:] + [POISON], V[1:] + [POISON]
            ge = j + d_hi - fc
            assert ge >= 0
            if ge < F:
                D[ge] = V[ge] = MARK                         # rule 2: the cell above the right edge, read through V and D
            # the cell left of the frame
            e = j - (c0 - d_hi)
            if s == 0 and jd <= 0:
                feed, kind = dict(z=max(M[r], A[r]), b=B[r], from_a=True, zs=Z, bs=Z), BORDER
                assert (M[r], B[r]) == (fl, fl) and not moving
            elif s > 0 and 0 <= e < width:
                assert hand_in[e] is not POISON, ("a hand-off entry that was never written", s, j, e)
                feed, kind = hand_in[e], HANDOFF
                assert not moving and (feed["z"], feed["b"]) == (max(M[r + c0], A[r + c0]), B[r + c0]), (s, j)
            else:
                feed, kind = nothing, NOTHING
                assert s == 0 or e >= width                  # (c0, j) is left of the band from here on
            if s == 0:
                cover["feeds0"].add(MOVING if moving else kind)
            dprev = bound_d
            bound_d = boundary(feed, j)                      # the feed becomes the up-left of position 0 on the next row
            free_row, forced = no_end and j == lb, ngb and j != lb
            n_row = min(cend, j + d_hi) - fc + 1
            assert 1 <= n_row <= F, (s, j, n_row)
            nD, nV = [POISON] * F, [POISON] * F              # rule 4: positions without a band cell of this strip
            run, zl = None, feed
            cells = [None] * F
            for g in range(n_row):
                x = fc + g
                m, av, bv = M[r + x], A[r + x], B[r + x]
                a_ok = (not nga) or x == la
                pd, pu = r - W_ + x - 1, r - W_ + x
                sc_, is_match = look(a[x - 1], b[j - 1])
                eq = fa[x - 1] == fb[j - 1]
                assert dprev is not POISON, ("D of the up-left", s, x, j)
                if (no_mm and not is_match) or max(M[pd], A[pd], B[pd]) + sc_ < fl:
                    ms = MARK
                else:
                    ms = (dprev[0] + eq, dprev[1] + (not eq), dprev[2])
                if no_end and x == la:
                    as_ = D[g]
                elif not a_ok or max(max(M[pu], B[pu]) + open1, A[pu] + ext) < fl:
                    as_ = MARK
                else:
                    as_ = V[g]
                if forced:
                    bs = MARK
                else:
                    step = 0 if free_row else ext
                    cand = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), zl["zs"])
                    if not free_row and fl > cand[0]:
                        cand = (fl, 0, MARK)                 # clamped: the floor loses a tie to every candidate
                    if g == 0:
                        cand = merge((feed["b"] + step, 1, feed["bs"]), cand)
                    if run is not None:
                        cand = merge((run[0] + step, run[1], run[2]), cand)
                    run = cand
                    assert run[0] == bv, (s, x, j, run, bv)
                    bs = run[2]
                assert POISON not in (ms, as_, bs), (s, x, j)      # a band cell never reads a position without one
                from_a = a_ok and av >= m
                zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
                cells[g] = dict(z=zl["z"], b=bv, from_a=from_a, zs=zl["zs"], bs=bs)
                mb = max(m, bv)
                low = bs if (not forced and bv >= m) else ms
                nD[g] = as_ if (a_ok and av >= mb) else low
                nV[g] = as_ if (a_ok and av + ext >= mb + open1) else low
                dprev = D[g]
            D, V = nD, nV
            if right_rows and j + d_hi >= c0 + F:            # my last column is in the band on this row: entry [row - e_out0]
                out = cells[c0 + F - fc]
                assert out is not None, ("the strip's last column holds no cell", s, j)
                eo = j - (c0 + F - d_hi)
                assert 0 <= eo < width and hand_out[eo] is POISON
                hand_out[eo] = out
                cover["entries"] += 1
                cover["marked"] += out["zs"][2] or out["bs"][2]
                cover["from_a"] += out["from_a"]
        if s > 0 and phases == {STANDING, MOVING}:
            cover["both_phases"] += 1
        if c0 + F >= la:                                     # the last strip: column len_a in the last row's frame
            at = la - max(c0 + 1, lb + d_lo)
            if lb == 0:
                result = Z                                   # row 0's border cell, as start_strip left it
            else:
                assert jf <= jl == lb and 0 <= at < F and D[at] is not POISON
                result = D[at]
        hand_in = hand_out
    m, mm, mark = result
    return (score, m, mm), mark, cover


def walk_crosses_seam(ra: bytes, rb: bytes, la: int, S: int) -> bool:
    """Whether the cells (x, y) with x > 0 and y > 0 that the alignment (ra, rb) passes through -- the part of the walk that is
    counted -- have columns in more than one strip of S columns."""
    x = y = 0
    strips = set()
    for p, q in zip(ra, rb):
        x += p != 0x2D
        y += q != 0x2D
        if x > 0 and y > 0:
            strips.add((x - 1) // S)
    return len(strips) > 1


def long_pairs(seed: int, n: int, alpha: bytes, lo: int = 15, hi: int = 40):
    """[(a, b, w)]: n relatives of lo .. hi letters, at least three strips at S = 7, alternately len_a < len_b and len_a > len_b,
    w from 0 to 12."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        a = bytes(rng.choice(alpha) for _ in range(rng.randrange(lo, hi + 1)))
        b = BL.mutate(rng, a, 0.25, alpha)
        tail = bytes(rng.choice(alpha) for _ in range(1 + rng.randrange(9)))
        a, b = (a, b + tail) if len(out) % 2 == 0 else (a + tail, b)
        if len(b) < lo or len(a) < lo or (len(a) < len(b)) != (len(out) % 2 == 0):
            continue
        out.append((a, b, rng.randrange(13)))
    return out


def definition_cases():
    """[(the ten numbers of a scoring's init, [(a, b, w)])] of the GPU tier's definition test: the 32 flag combinations, eight
    mixed-case pairs of up to 300 letters each -- seven in ten relatives with 20 % edits -- at w = 0 .. 40, or 150."""
    import itertools
    rng = random.Random(1501)
    alpha = b"ACGTacgt"
    seq = lambda n: bytes(rng.choice(alpha) for _ in range(n))
    out = []
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        both_no_gaps = flags[2] and flags[3]
        init = [1, -6 if both_no_gaps else -2, -4, -1] if idx % 2 else [2, -7 if both_no_gaps else -3, 0, -2]
        triples = []
        for k in range(8):
            a = seq(rng.randrange(0, 301))
            b = BL.mutate(rng, a, 0.2, alpha)[:300] if rng.random() < 0.7 else seq(rng.randrange(0, 301))
            triples.append((a, b, 150 if (idx + k) % 11 == 0 else rng.randrange(0, 41)))
        out.append(([*init, *flags, 0], triples))
    return out
