"""The banded NW definition, restated in Python for the tests (include/seqalign_hip.h, "banded NW").

fill(sc, a, b, band) is the reference's recurrence (NW, borders included) for any scoring -- all five flags, case
folding, substitution tables, wildcards and mutations, through a table of the oracle's orc_scoring_lookup -- in which every cell
outside the band holds the NW floor in all three matrices.
expected(sc, a, b, w) walks those matrices with the oracle's needleman_wunsch end pick and alignment_reverse_move
(orclib.oracle_nw_traceback): (score, a, b), or None when there is no alignment inside the band."""
import ctypes as C

import numpy as np

import orclib as O

INT_MIN = -2 ** 31


def band_of(la: int, lb: int, w: int):
    """(d_lo, d_hi) of a pair: cell (i, j) is in the band iff d_lo <= i - j <= d_hi."""
    return max(-lb, min(0, la - lb) - w), min(la, max(0, la - lb) + w)


def width_of(la: int, lb: int, w: int) -> int:
    d_lo, d_hi = band_of(la, lb, w)
    return d_hi - d_lo + 1


def w_for_width(la: int, lb: int, width: int) -> int:
    """The w whose band is `width` diagonals wide (width >= |la - lb| + 1, same parity rule: width = |la - lb| + 1 + 2 w
    before the clamp), or None."""
    extra = width - abs(la - lb) - 1
    if extra < 0:
        return None
    for w in (extra // 2, extra // 2 + 1, extra):
        if width_of(la, lb, w) == width:
            return w
    for w in range(0, extra + 1):
        if width_of(la, lb, w) == width:
            return w
    return None


_TABLES = {}


def scoring_table(sc, a: bytes, b: bytes):
    """The oracle's orc_scoring_lookup as tables, kept per scoring and filled in for the letters of a and b on first use:
    (score, is_match, arrays), the first two as table[seq_b's letter][seq_a's letter] with score None where the pair has
    none (ORC_ERR_UNKNOWN_PAIR), arrays = (score with 0 for None, is_match, has a score) as numpy.  Case folding is the
    lookup's own, so the tables are indexed by the letters as they stand in the sequences."""
    key = bytes(sc)
    hit = _TABLES.get(key)
    if hit is None:
        hit = _TABLES[key] = ([[None] * 128 for _ in range(128)], [[False] * 128 for _ in range(128)],
                              (np.zeros((128, 128), np.int64), np.zeros((128, 128), bool), np.zeros((128, 128), bool)), set())
    score, same, (score_np, same_np, known_np), done = hit
    todo = {(x, y) for x in set(a) for y in set(b)} - done
    if todo:
        lk = O.oracle().orc_scoring_lookup
        s, m = C.c_int(0), C.c_int(0)
        for x, y in todo:
            if lk(C.byref(sc), C.c_char(bytes([x])), C.c_char(bytes([y])), C.byref(s), C.byref(m)) == 0:
                score[y][x] = score_np[y, x] = s.value
                known_np[y, x] = True
            same[y][x] = same_np[y, x] = bool(m.value)
        done |= todo
    return hit[:3]


def _borders(sc, la, lb, d_lo, d_hi, mn):
    """Row 0 and column 0 of the three matrices (alignment.c:46-81), the floor outside the band."""
    M = np.full((lb + 1, la + 1), mn, np.int64)
    A, B = M.copy(), M.copy()
    M[0, 0] = A[0, 0] = B[0, 0] = 0
    i = np.arange(1, la + 1)
    i = i[(d_lo <= i) & (i <= d_hi)]
    B[0, i] = 0 if sc.no_start_gap_penalty else sc.gap_open + i * sc.gap_extend
    j = np.arange(1, lb + 1)
    j = j[(d_lo <= -j) & (-j <= d_hi)]
    A[j, 0] = 0 if sc.no_start_gap_penalty else sc.gap_open + j * sc.gap_extend
    return M, A, B


def fill_unknown(sc, a: bytes, b: bytes, band=None, border_feed=False):
    """M, A, B (int32, pitch len(a) + 1) and the band cells (i, j), in row order, whose letters have no score: such a cell
    keeps the floor in M.  band = (d_lo, d_hi) or None for the whole matrix.
    border_feed = True is NOT the definition: the cell left of a row's first band cell, below the border column's last band
    cell, then reads as the border column's value of that row instead of the floor -- what a fill that never stops feeding
    the border would compute.  The tests use it to show, on the reference alone, that a pair would notice.

    One row at a time in numpy.  M and A read the row above only.  B[i] = max(src[i], B[i - 1] + e) with
    src[i] = max(floor, max(M, A)[i - 1] + o) unrolls to max over i' <= i of src[i'] + (i - i') e -- a running maximum of
    src[i'] - i' e -- exactly, for either sign of e, because the floor is inside src.  fill_cells is the same recurrence cell by
    cell; test_band_argument_cpu.py holds the two together."""
    la, lb = len(a), len(b)
    go, ge = sc.gap_open + sc.gap_extend, sc.gap_extend
    mn = INT_MIN + abs(sc.min_penalty)
    d_lo, d_hi = (-(lb + 1), la + 1) if band is None else band
    M, A, B = _borders(sc, la, lb, d_lo, d_hi, mn)
    score, same, known = scoring_table(sc, a, b)[2]
    ca, cb = np.frombuffer(a, np.uint8).astype(np.intp), np.frombuffer(b, np.uint8).astype(np.intp)
    no_mm, no_end, no_ga, no_gb = bool(sc.no_mismatches), bool(sc.no_end_gap_penalty), bool(sc.no_gaps_in_a), bool(sc.no_gaps_in_b)
    unknown = []
    for j in range(1, lb + 1):
        i0, i1 = max(1, j + d_lo), min(la, j + d_hi)
        if i0 > i1:
            continue
        x, y = ca[i0 - 1:i1], cb[j - 1]
        cur, left, diag = slice(i0, i1 + 1), slice(i0 - 1, i1), slice(i0 - 1, i1)
        m = np.maximum(np.maximum(np.maximum(M[j - 1, diag], A[j - 1, diag]), B[j - 1, diag]) + score[y, x], mn)
        if no_mm:
            m = np.where(same[y, x], m, mn)
        ok = known[y, x]
        if not ok.all():
            m = np.where(ok, m, mn)
            unknown += [(i0 + int(t), j) for t in np.nonzero(~ok)[0]]
        M[j, cur] = m
        Mu, Au, Bu = M[j - 1, cur], A[j - 1, cur], B[j - 1, cur]
        if no_ga:
            av = np.full(i1 - i0 + 1, mn, np.int64)
        else:
            av = np.maximum(np.maximum(np.maximum(Mu, Bu) + go, Au + ge), mn)
        if i1 == la:                                   # the rightmost column
            if no_end:
                av[-1] = max(Mu[-1], Au[-1], Bu[-1])
            elif no_ga:
                av[-1] = max(Mu[-1] + go, Au[-1] + ge, Bu[-1] + go, mn)
        A[j, cur] = av
        if j == lb and no_end:
            o, e = 0, 0
        elif (not no_gb) or j == lb:
            o, e = go, ge
        else:
            continue                                   # B stays at the floor
        t = np.arange(i1 - i0 + 1)
        z = np.maximum(M[j, left], A[j, left])
        if border_feed and j + d_lo >= 1:
            z[0] = max(mn, 0 if sc.no_start_gap_penalty else sc.gap_open + j * sc.gap_extend)
        cand = np.maximum(z + o, mn) - t * e
        cand[0] = max(cand[0], B[j, i0 - 1] + e)
        B[j, cur] = np.maximum.accumulate(cand) + t * e
    return M.astype(np.int32).ravel(), A.astype(np.int32).ravel(), B.astype(np.int32).ravel(), unknown


def fill(sc, a: bytes, b: bytes, band=None):
    """M, A, B of fill_unknown."""
    return fill_unknown(sc, a, b, band)[:3]


def fill_cells(sc, a: bytes, b: bytes, band=None):
    """fill_unknown's four values, cell by cell in plain Python as alignment.c:28-168 reads: slow, and nothing to get wrong."""
    la, lb = len(a), len(b)
    W = la + 1
    go, ge = sc.gap_open + sc.gap_extend, sc.gap_extend
    mn = INT_MIN + abs(sc.min_penalty)
    M = [mn] * ((lb + 1) * W)
    A = list(M)
    B = list(M)
    d_lo, d_hi = (-(lb + 1), la + 1) if band is None else band
    M[0] = A[0] = B[0] = 0
    for i in range(1, W):
        if d_lo <= i <= d_hi:
            B[i] = 0 if sc.no_start_gap_penalty else sc.gap_open + i * ge
    for j in range(1, lb + 1):
        if d_lo <= -j <= d_hi:
            A[j * W] = 0 if sc.no_start_gap_penalty else sc.gap_open + j * ge
    score, same = scoring_table(sc, a, b)[:2]
    no_mm, no_end, no_ga, no_gb = bool(sc.no_mismatches), bool(sc.no_end_gap_penalty), bool(sc.no_gaps_in_a), bool(sc.no_gaps_in_b)
    unknown = []
    for j in range(1, lb + 1):
        srow, mrow = score[b[j - 1]], same[b[j - 1]]
        for i in range(max(1, j + d_lo), min(la, j + d_hi) + 1):
            c = j * W + i
            s = srow[a[i - 1]]
            ul, up, lf = c - W - 1, c - W, c - 1
            if s is None:
                unknown.append((i, j))
            elif no_mm and not mrow[a[i - 1]]:
                M[c] = mn
            else:
                M[c] = max(M[ul] + s, A[ul] + s, B[ul] + s, mn)
            if i == la and no_end:
                A[c] = max(M[up], A[up], B[up])
            elif (not no_ga) or i == la:
                A[c] = max(M[up] + go, A[up] + ge, B[up] + go, mn)
            else:
                A[c] = mn
            if j == lb and no_end:
                B[c] = max(M[lf], A[lf], B[lf])
            elif (not no_gb) or j == lb:
                B[c] = max(M[lf] + go, A[lf] + go, B[lf] + ge, mn)
            else:
                B[c] = mn
    as_i32 = lambda X: np.array(X, np.int64).astype(np.int32)
    return as_i32(M), as_i32(A), as_i32(B), unknown


def end_value(M, A, B) -> int:
    """What the score call returns: the largest of the three at (len_a, len_b)."""
    return int(max(M[-1], A[-1], B[-1]))


def expected_both(sc, a: bytes, b: bytes, w: int, band=None):
    """(what the score call returns, what the align call returns or None) from one fill; band = (d_lo, d_hi) replaces w's."""
    M, A, B = fill(sc, a, b, band or band_of(len(a), len(b), w))
    rc, score, ra, rb = O.oracle_nw_traceback(sc, a, b, M, A, B)
    return end_value(M, A, B), (None if rc != 0 else (score, ra, rb))


def expected(sc, a: bytes, b: bytes, w: int):
    """(score, gapped a, gapped b) of the banded alignment, or None: no alignment inside the band."""
    return expected_both(sc, a, b, w)[1]


def expected_score(sc, a: bytes, b: bytes, w: int, band=None, border_feed=False) -> int:
    return end_value(*fill_unknown(sc, a, b, band or band_of(len(a), len(b), w), border_feed)[:3])


def excursion(ra: bytes, rb: bytes):
    """(lowest, highest) i - j along an alignment given as its two gapped strings, the start cell (0, 0) included."""
    i = j = lo = hi = 0
    for x, y in zip(ra, rb):
        if x != 0x2D:
            i += 1
        if y != 0x2D:
            j += 1
        lo, hi = min(lo, i - j), max(hi, i - j)
    return lo, hi


def smallest_band(ra: bytes, rb: bytes, la: int, lb: int) -> int:
    """The smallest w whose band holds the alignment."""
    lo, hi = excursion(ra, rb)
    return max(0, min(0, la - lb) - lo, hi - max(0, la - lb))


def in_band(ra: bytes, rb: bytes, la: int, lb: int, w: int) -> bool:
    d_lo, d_hi = band_of(la, lb, w)
    lo, hi = excursion(ra, rb)
    return d_lo <= lo and hi <= d_hi


def mutate(rng, a: bytes, p: float, alphabet: bytes = b"ACGT") -> bytes:
    """Edits in equal thirds: deletions, insertions, substitutions, at rate p per letter."""
    out = bytearray()
    for ch in a:
        r = rng.random()
        if r < p / 3:
            continue
        if r < 2 * p / 3:
            out += bytes([ch, rng.choice(alphabet)])
            continue
        if r < p:
            out.append(rng.choice(alphabet))
            continue
        out.append(ch)
    return bytes(out)
