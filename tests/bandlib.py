"""The banded NW definition, restated in Python for the tests (include/seqalign_hip.h, "banded NW").

fill(sc, a, b, band) is the reference's recurrence (NW, borders included) for plain match / mismatch scorings --
all five flags, case folding -- in which every cell outside the band holds the NW floor in all three matrices.
expected(sc, a, b, w) walks those matrices with the oracle's needleman_wunsch end pick and alignment_reverse_move
(orclib.oracle_nw_traceback): (score, a, b), or None when there is no alignment inside the band."""
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


def fill(sc, a: bytes, b: bytes, band=None):
    """M, A, B (int32, pitch len(a) + 1).  band = (d_lo, d_hi) or None for the whole matrix."""
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
    if sc.case_sensitive:
        al, bl = a, b
    else:
        al, bl = a.lower(), b.lower()
    no_mm, no_end, no_ga, no_gb = bool(sc.no_mismatches), bool(sc.no_end_gap_penalty), bool(sc.no_gaps_in_a), bool(sc.no_gaps_in_b)
    match, mismatch = sc.match, sc.mismatch
    for j in range(1, lb + 1):
        cb = bl[j - 1]
        for i in range(max(1, j + d_lo), min(la, j + d_hi) + 1):
            c = j * W + i
            ism = al[i - 1] == cb
            s = match if ism else mismatch
            ul, up, lf = c - W - 1, c - W, c - 1
            if no_mm and not ism:
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
    return np.array(M, np.int64).astype(np.int32), np.array(A, np.int64).astype(np.int32), np.array(B, np.int64).astype(np.int32)


def end_value(M, A, B) -> int:
    """What the score call returns: the largest of the three at (len_a, len_b)."""
    return int(max(M[-1], A[-1], B[-1]))


def expected(sc, a: bytes, b: bytes, w: int):
    """(score, gapped a, gapped b) of the banded alignment, or None: no alignment inside the band."""
    M, A, B = fill(sc, a, b, band_of(len(a), len(b), w))
    rc, score, ra, rb = O.oracle_nw_traceback(sc, a, b, M, A, B)
    if rc != 0:
        return None
    return score, ra, rb


def expected_score(sc, a: bytes, b: bytes, w: int) -> int:
    return end_value(*fill(sc, a, b, band_of(len(a), len(b), w)))


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
