"""Helpers of the NW gap-run tests (seqalign_nw_gaps_batch / _cross / _banded / _banded_wide).  Not a test module.

want_gaps           what the unbanded calls must return per pair, from orclib.oracle_nw's strings and swgaplib.gap_runs:
                    (score, gap_runs_a, gap_runs_b), None for a pair whose traceback fails;
band_want           the same over the banded matrices (bandnwstatlib.want_walked: bandlib's banded end value and the oracle's
                    walk over the banded matrices), None where no alignment lies inside the band;
got_gaps            the calls' three arrays as a list of such tuples;
border_run          the pair of a border cell, whatever the state: (0, 0) at (0, 0), (0, 1) at (x, 0), (1, 0) at (0, y) -- the
                    reference leaves its loop there and emits the rest as ONE run of gap columns;
forward             the DEFINITION the kernels rest on, in pure Python over the oracle's matrices:
                    run(cell, S) is border_run on the border, else run(the predecessor statlib.step picks), plus one in a gap
                    state's own word UNLESS the picked predecessor is the same gap state in a cell that is not on the border;
                    a state without a predecessor (and every state of a cell outside the band) carries the sticky mark.
                    flat_border: the deliberately wrong model that puts (0, 0) on the whole border, as the identity counts do;
walk                the same by walking back from the end pick, step by step; also says whether the walk ends in a border run;
kernel_model        the sweep's own shape on the CPU (sa_nw_gaps.hpp): statlib.kernel_model with the payload of a state
                    (gap_runs_a, gap_runs_b, mark), every feed and hand-off RAW and the increment decided in the consuming
                    cell; strips hand on {max(M, A), B, whether A's, the two payloads};
frame_model         bandnwstatlib.frame_model in the same form: the NW band frame's bookkeeping (sa_band_nw_frame.hpp); a
                    position that holds no band cell carries POISON;
deleted_inserted    the constructed long pair: a sequence against itself with one block deleted and one inserted.
"""
from __future__ import annotations

import bandlib as BL
import bandnwstatlib as BN
import orclib as O
import statlib as ST
import swgaplib as SG

MATCH, GAP_A, GAP_B = ST.MATCH, ST.GAP_A, ST.GAP_B
WALKER, REVERSED = ST.WALKER, ST.REVERSED
NO_WALK = ST.NO_WALK
POISON = None
MARK = (0, 0, True)                # what is counted beside the mark is never read: every marked payload compares as this one
BORDER, STOPPED, MOVING = BN.BORDER, BN.STOPPED, BN.MOVING


def want_one(osc, a: bytes, b: bytes):
    rc, s, ra, rb = O.oracle_nw(osc, a, b)
    if rc:
        return None if rc == ST.E_TRACEBACK else ("rc", rc)
    return (s,) + SG.gap_runs(ra, rb)


def want_gaps(osc, pairs):
    """[(score, gap_runs_a, gap_runs_b) | None] per (a, b)."""
    return [want_one(osc, a, b) for a, b in pairs]


def band_want(osc, a: bytes, b: bytes, w: int):
    """(score, gap_runs_a, gap_runs_b) over the banded matrices, or None: no alignment inside the band."""
    both = BN.want_walked(osc, a, b, w)
    if both is None:
        return None
    stats, walked = both
    return (stats[0],) + SG.gap_runs(walked[1], walked[2])


def got_gaps(res):
    return [tuple(int(x[p]) for x in res) for p in range(len(res[0]))]


def begins_with_gap(osc, a: bytes, b: bytes) -> bool:
    """Whether the oracle's alignment begins with a gap column: the walk ends in a border run."""
    rc, _, ra, rb = O.oracle_nw(osc, a, b)
    assert rc == 0
    return bool(ra) and (ra[:1] == b"-" or rb[:1] == b"-")


# ------------------------------------------------------------------------------------------------- the definition ---
def border_run(x: int, y: int, flat: bool = False):
    if flat or (x == 0 and y == 0):
        return (0, 0, False)
    return (0, 1, False) if y == 0 else (1, 0, False)


def _bump(pay, st):
    if pay[2]:
        return MARK
    return (pay[0] + 1, pay[1], False) if st == GAP_A else (pay[0], pay[1] + 1, False)


def _blocked(osc, look, ca, cb):
    return bool(osc.no_mismatches) and not look(ca, cb)[1]


def forward(osc, a: bytes, b: bytes, priority=WALKER, mats=None, band=None, flat_border=False):
    """Returns (result, run): result = (score, gap_runs_a, gap_runs_b) or NO_WALK; run[state][y * W + x] = (gap_runs_a,
    gap_runs_b, marked) of the walk that starts there.  band = (d_lo, d_hi) with the banded matrices in mats: a cell outside
    the band holds the mark in all three states."""
    la, lb = len(a), len(b)
    W_ = la + 1
    M, A, B = mats or ST.matrices(osc, a, b)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = ST.Lookup(osc)
    run = {st: [None] * (W_ * (lb + 1)) for st in (MATCH, GAP_A, GAP_B)}
    for y in range(lb + 1):
        for x in range(W_):
            at = y * W_ + x
            outside = band is not None and not (band[0] <= x - y <= band[1])
            for st in (MATCH, GAP_A, GAP_B):
                if x == 0 or y == 0:
                    run[st][at] = MARK if outside else border_run(x, y, flat_border)
                    continue
                pred = None if outside else ST.step(osc, vals, a, b, x, y, st, look, priority)
                if st == MATCH and _blocked(osc, look, a[x - 1], b[y - 1]):
                    pred = None
                if pred is None:
                    run[st][at] = MARK
                    continue
                s2, nx, ny = pred
                got = run[s2][ny * W_ + nx]
                if st != MATCH and not (s2 == st and nx > 0 and ny > 0):
                    got = _bump(got, st)
                run[st][at] = MARK if got[2] else got
    end = W_ * (lb + 1) - 1
    st, score = ST.end_pick(M, A, B, end)
    ra, rb, mark = run[st][end]
    return (NO_WALK if mark else (score, ra, rb)), run


def walk(osc, a: bytes, b: bytes, priority=WALKER, mats=None):
    """((score, gap_runs_a, gap_runs_b) or NO_WALK, whether the walk ends in a border run) by walking back from the end pick."""
    la, lb = len(a), len(b)
    W_ = la + 1
    M, A, B = mats or ST.matrices(osc, a, b, as_lists=False)
    vals = {MATCH: M, GAP_A: A, GAP_B: B}
    look = ST.Lookup(osc)
    st, score = ST.end_pick(M, A, B, W_ * (lb + 1) - 1)
    x, y, runs = la, lb, [0, 0]
    while x > 0 and y > 0:
        pred = ST.step(osc, vals, a, b, x, y, st, look, priority)
        if pred is None:
            return NO_WALK, False
        s2, nx, ny = pred
        if st != MATCH and not (s2 == st and nx > 0 and ny > 0):
            runs[0 if st == GAP_A else 1] += 1
        st, x, y = pred
    runs[0] += y > 0                                        # the rest of seq_b against gaps: one run in string a
    runs[1] += x > 0
    return (score, runs[0], runs[1]), (x > 0 or y > 0)


# ---------------------------------------------------------------------------------------------- the kernel's shape ---
def _norm(pay):
    return MARK if pay[2] else pay


def _merge(l, r):                      # l lies left of r: r wins a tie only as an opening from A (nm = 1)
    return l if l[0] >= r[0] + r[1] else r


def _gap_a_state(src, ext_wins, above_inner):
    """gap_a's pair in the consuming cell: the raw feed + 1 unless the extension wins it and the row above is not row 0."""
    return _norm(src) if (ext_wins and above_inner) else _bump(src, GAP_A)


def _result(score, pay):
    return NO_WALK if pay[2] else (score, pay[0], pay[1])


def kernel_model(osc, a: bytes, b: bytes, strip_cols: int = 1 << 30, run=None):
    """(score, gap_runs_a, gap_runs_b) or NO_WALK the way the kernel finds it.  run: forward()'s payloads -- every state of every
    cell is then compared with the definition."""
    la, lb = len(a), len(b)
    W_ = la + 1
    M, A, B = ST.matrices(osc, a, b)
    st, score = ST.end_pick(M, A, B, W_ * (lb + 1) - 1)
    if la == 0:
        return _result(score, border_run(0, lb))            # write_border
    fl = ST.floor_of(osc)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, nga, ngb = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_a), bool(osc.no_gaps_in_b)
    look = ST.Lookup(osc)
    D = [border_run(x, 0) for x in range(W_)]               # row 0: start_strip's (0, 1), (0, 0) as the up-left of column 1
    V = list(D)

    for y in range(1, lb + 1):
        r = y * W_
        free_row, forced = no_end and y == lb, ngb and y != lb
        nD, nV = [border_run(0, y)] + [None] * la, [border_run(0, y)] + [None] * la
        feed = dict(z=max(M[r], A[r]), b=B[r], from_a=A[r] >= M[r], zs=border_run(0, y), bs=border_run(0, y))   # the border column
        for i0 in range(0, la, strip_cols):
            hi = min(la, i0 + strip_cols)
            chain, zl, out = None, feed, None
            for x in range(i0 + 1, hi + 1):
                m, av, bv = M[r + x], A[r + x], B[r + x]
                a_ok = (not nga) or x == la
                pd, pu = r - W_ + x - 1, r - W_ + x
                s = look(a[x - 1], b[y - 1])[0]
                if _blocked(osc, look, a[x - 1], b[y - 1]) or max(M[pd], A[pd], B[pd]) + s < fl:
                    ms = MARK
                else:
                    ms = _norm(D[x - 1])                     # the match state adds nothing
                yv, ap = max(M[pu], B[pu]), A[pu]
                if no_end and x == la:
                    as_ = _gap_a_state(D[x], ap >= yv, y > 1)
                elif not a_ok or max(yv + open1, ap + ext) < fl:
                    as_ = MARK
                else:
                    as_ = _gap_a_state(V[x], ap + ext >= yv + open1, y > 1)
                if forced:
                    bs = MARK
                else:
                    step_ = 0 if free_row else ext
                    w = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), _bump(zl["zs"], GAP_B))    # an opening
                    if not free_row and fl > w[0]:
                        w = (fl, 0, MARK)                    # clamped: the floor loses a tie to every candidate
                    if x == i0 + 1:                          # the carry: raw from a strip, + 1 out of the border column
                        carried = _bump(feed["bs"], GAP_B) if i0 == 0 else _norm(feed["bs"])
                        w = _merge((feed["b"] + step_, 1, carried), w)
                    if chain is not None:
                        w = _merge((chain[0] + step_, chain[1], chain[2]), w)
                    chain = w
                    assert chain[0] == bv, (x, y, chain, bv)
                    bs = chain[2]
                if run is not None:
                    assert run[MATCH][r + x] == ms, ("M", x, y, ms, run[MATCH][r + x])
                    if a_ok:
                        assert run[GAP_A][r + x] == as_, ("A", x, y, as_, run[GAP_A][r + x])
                    if not forced:
                        assert run[GAP_B][r + x] == bs, ("B", x, y, bs, run[GAP_B][r + x])
                from_a = a_ok and av >= m
                zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
                mb = max(m, bv)
                low = bs if (not forced and bv >= m) else ms
                nD[x] = as_ if (a_ok and av >= mb) else low
                nV[x] = as_ if (a_ok and av + ext >= mb + open1) else low
                out = dict(z=zl["z"], b=bv, from_a=from_a, zs=zl["zs"], bs=bs)
            if hi < la:                                      # what this strip hands the next one: raw
                feed = out
                zwins = forced or ((feed["z"] >= feed["b"]) if feed["from_a"] else (feed["z"] > feed["b"]))
                assert nD[hi] == (feed["zs"] if zwins else feed["bs"]), (hi, y)
        D, V = nD, nV
    return _result(score, D[la])


def frame_model(osc, a: bytes, b: bytes, w: int, F: int = 8, run=None):
    """((score, gap_runs_a, gap_runs_b) or NO_WALK, the phases of the feed the rows went through) the way
    band_nw_payload_rows_kernel finds them over NwGapSweep with a frame of F positions.  run: the definition's payloads over the
    banded matrices (forward with mats and band) -- every band cell's states are then compared with them."""
    la, lb = len(a), len(b)
    W_ = la + 1
    d_lo, d_hi = BL.band_of(la, lb, w)
    assert d_hi - d_lo + 1 <= F
    M, A, B = (X.tolist() for X in BL.fill(osc, a, b, (d_lo, d_hi)))
    score = ST.end_pick(M, A, B, W_ * (lb + 1) - 1)[1]
    if la == 0:                                              # the border column is the whole matrix
        return _result(score, border_run(0, lb)), set()
    fl = ST.floor_of(osc)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, nga, ngb = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_a), bool(osc.no_gaps_in_b)
    look = ST.Lookup(osc)

    # row 0: the frame stands at column 1; columns 1 .. d_hi are band cells of the border
    D = [border_run(1 + g, 0) if 1 + g <= min(la, d_hi) else POISON for g in range(F)]
    V = list(D)
    bound_d = border_run(0, 0)
    phases = set()
    for j in range(1, lb + 1):
        r = j * W_
        fc = max(1, j + d_lo)
        phase = BORDER if j + d_lo <= 0 else STOPPED if j + d_lo == 1 else MOVING
        phases.add(phase)
        if phase == MOVING:                                  # rule 1: the frame moves
            bound_d = D[0]
            D, V = D[1:] + [POISON], V[1:] + [POISON]
        ge = j + d_hi - fc
        assert 0 <= ge < F
        D[ge] = V[ge] = MARK                                 # rule 2: the cell above the right edge, read through V and D
        if phase == BORDER:
            feed = dict(z=max(M[r], A[r]), b=B[r], from_a=True, zs=border_run(0, j), bs=border_run(0, j))
            assert (M[r], B[r]) == (fl, fl)
        else:
            feed = dict(z=fl, b=fl, from_a=False, zs=MARK, bs=MARK)
        dprev = bound_d
        free_row, forced = no_end and j == lb, ngb and j != lb
        zwins = forced or ((feed["z"] >= feed["b"]) if feed["from_a"] else (feed["z"] > feed["b"]))
        bound_d = feed["zs"] if zwins else feed["bs"]        # the feed becomes the up-left of position 0 on the next row
        n_row = min(la, j + d_hi) - fc + 1
        assert 1 <= n_row <= F
        nD, nV = [POISON] * F, [POISON] * F                  # rule 4: positions without a band cell
        chain, zl = None, feed
        for g in range(n_row):
            x = fc + g
            m, av, bv = M[r + x], A[r + x], B[r + x]
            a_ok = (not nga) or x == la
            pd, pu = r - W_ + x - 1, r - W_ + x
            s = look(a[x - 1], b[j - 1])[0]
            assert dprev is not POISON, ("D of the up-left", x, j)
            if _blocked(osc, look, a[x - 1], b[j - 1]) or max(M[pd], A[pd], B[pd]) + s < fl:
                ms = MARK
            else:
                ms = _norm(dprev)
            yv, ap = max(M[pu], B[pu]), A[pu]
            if no_end and x == la:
                assert D[g] is not POISON, ("D above", x, j)
                as_ = _gap_a_state(D[g], ap >= yv, j > 1)
            elif not a_ok or max(yv + open1, ap + ext) < fl:
                as_ = MARK
            else:
                assert V[g] is not POISON, ("V above", x, j)
                as_ = _gap_a_state(V[g], ap + ext >= yv + open1, j > 1)
            if forced:
                bs = MARK
            else:
                step = 0 if free_row else ext
                cand = (zl["z"] + (0 if free_row else open1), int(zl["from_a"]), _bump(zl["zs"], GAP_B))
                if not free_row and fl > cand[0]:
                    cand = (fl, 0, MARK)                     # clamped: the floor loses a tie to every candidate
                if g == 0:                                   # col0 == 0: the cell left of column 1 is the border column's
                    carried = _bump(feed["bs"], GAP_B) if fc == 1 else _norm(feed["bs"])
                    cand = _merge((feed["b"] + step, 1, carried), cand)
                if chain is not None:
                    cand = _merge((chain[0] + step, chain[1], chain[2]), cand)
                chain = cand
                assert chain[0] == bv, (x, j, chain, bv)
                bs = chain[2]
            if run is not None:
                at = r + x
                assert run[MATCH][at] == ms, ("M", x, j, ms, run[MATCH][at])
                if a_ok:
                    assert run[GAP_A][at] == as_, ("A", x, j, as_, run[GAP_A][at])
                if not forced:
                    assert run[GAP_B][at] == bs, ("B", x, j, bs, run[GAP_B][at])
            from_a = a_ok and av >= m
            zl = dict(z=max(m, av), from_a=from_a, zs=as_ if from_a else ms)
            mb = max(m, bv)
            low = bs if (not forced and bv >= m) else ms
            nD[g] = as_ if (a_ok and av >= mb) else low
            nV[g] = as_ if (a_ok and av + ext >= mb + open1) else low
            dprev = D[g]
        D, V = nD, nV
    at = la - max(1, lb + d_lo)
    assert 0 <= at < F and D[at] is not POISON
    return _result(score, D[at]), phases


# ----------------------------------------------------------------------------------------------------------- pairs ---
BLOCK_INIT = [1, -3, -5, -1]       # a gap of 40 costs 45, the flanks score thousands: one alignment, one run in each string


def deleted_inserted(rng, n: int = 6000, at_d: int = 2000, deleted: int = 40, at_i: int = 4000, inserted: int = 25):
    """(a, b) over ACGT: b is a without a[at_d : at_d + deleted] and with `inserted` letters put in at at_i (a run of T between
    a non-T pair, so that no letter of it extends a flank): under BLOCK_INIT the alignment has one run of '-' in each string."""
    a = bytearray(b"ACG"[i] for i in rng.below(3, n))
    return bytes(a), bytes(a[:at_d] + a[at_d + deleted:at_i] + b"T" * inserted + a[at_i:])
