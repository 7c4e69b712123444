"""The banded SW definition, restated in Python for the tests (include/seqalign_hip.h, "banded SW").

Pair bounds lo <= hi; cell (i, j) -- column i of seq_a, row j of seq_b -- is in the band iff lo <= i - j <= hi, the bounds
clipped to [-len_b, len_a].  fill(sc, a, b, band) is the reference's recurrence (is_sw = 1) for any scoring -- all
five flags, case folding, substitution tables, wildcards and mutations, through bandlib.scoring_table -- in which every cell
outside the band holds the SW floor, 0, in all three matrices (the SW borders are 0 as well).
expected(sc, a, b, lo, hi, min_score) is what the two calls return: the best match_scores cell in hit order and the oracle's
first hit (orclib.oracle_sw_hits, max_hits = 1) over those matrices."""
import numpy as np

import bandlib as BL
import orclib as O


def clip(la: int, lb: int, lo: int, hi: int):
    """The clipped band (d_lo, d_hi), or None when it is empty."""
    d_lo, d_hi = max(lo, -lb), min(hi, la)
    return None if d_lo > d_hi else (d_lo, d_hi)


def width_of(la: int, lb: int, lo: int, hi: int) -> int:
    band = clip(la, lb, lo, hi)
    return 0 if band is None else band[1] - band[0] + 1


def fill_unknown(sc, a: bytes, b: bytes, band=None):
    """M, A, B (int32, pitch len(a) + 1) and the band cells (i, j), in row order, whose letters have no score: such a cell
    keeps 0 in M.  band = (lo, hi) as the caller gives them, or None for the whole matrix.

    One row at a time in numpy, as bandlib.fill_unknown: B[i] = max(src[i], B[i - 1] + e) unrolls to a running maximum of
    src[i'] - i' e, exactly, because the floor is inside src.  fill_cells is the same recurrence cell by cell;
    test_band_sw_argument_cpu.py holds the two together."""
    la, lb = len(a), len(b)
    go, ge = sc.gap_open + sc.gap_extend, sc.gap_extend
    M = np.zeros((lb + 1, la + 1), np.int64)
    A, B = M.copy(), M.copy()
    unknown = []
    clipped = (-lb, la) if band is None else clip(la, lb, *band)
    if clipped is None:
        return M.astype(np.int32).ravel(), A.astype(np.int32).ravel(), B.astype(np.int32).ravel(), unknown
    d_lo, d_hi = clipped
    score, same, known = BL.scoring_table(sc, a, b)[2]
    ca, cb = np.frombuffer(a, np.uint8).astype(np.intp), np.frombuffer(b, np.uint8).astype(np.intp)
    no_mm, no_end, no_ga, no_gb = bool(sc.no_mismatches), bool(sc.no_end_gap_penalty), bool(sc.no_gaps_in_a), bool(sc.no_gaps_in_b)
    for j in range(1, lb + 1):
        i0, i1 = max(1, j + d_lo), min(la, j + d_hi)
        if i0 > i1:
            continue
        x, y = ca[i0 - 1:i1], cb[j - 1]
        cur, left, diag = slice(i0, i1 + 1), slice(i0 - 1, i1), slice(i0 - 1, i1)
        m = np.maximum(np.maximum(np.maximum(M[j - 1, diag], A[j - 1, diag]), B[j - 1, diag]) + score[y, x], 0)
        if no_mm:
            m = np.where(same[y, x], m, 0)
        ok = known[y, x]
        if not ok.all():
            m = np.where(ok, m, 0)
            unknown += [(i0 + int(t), j) for t in np.nonzero(~ok)[0]]
        M[j, cur] = m
        Mu, Au, Bu = M[j - 1, cur], A[j - 1, cur], B[j - 1, cur]
        if no_ga:
            av = np.zeros(i1 - i0 + 1, np.int64)
        else:
            av = np.maximum(np.maximum(np.maximum(Mu, Bu) + go, Au + ge), 0)
        if i1 == la:                                   # the rightmost column
            if no_end:
                av[-1] = max(Mu[-1], Au[-1], Bu[-1])
            elif no_ga:
                av[-1] = max(Mu[-1] + go, Au[-1] + ge, Bu[-1] + go, 0)
        A[j, cur] = av
        if j == lb and no_end:
            o, e = 0, 0
        elif (not no_gb) or j == lb:
            o, e = go, ge
        else:
            continue                                   # B stays at the floor
        t = np.arange(i1 - i0 + 1)
        z = np.maximum(M[j, left], A[j, left])
        cand = np.maximum(z + o, 0) - t * e
        cand[0] = max(cand[0], B[j, i0 - 1] + e)
        B[j, cur] = np.maximum.accumulate(cand) + t * e
    return M.astype(np.int32).ravel(), A.astype(np.int32).ravel(), B.astype(np.int32).ravel(), unknown


def fill(sc, a: bytes, b: bytes, band=None):
    """M, A, B of fill_unknown."""
    return fill_unknown(sc, a, b, band)[:3]


def fill_cells(sc, a: bytes, b: bytes, band=None):
    """fill_unknown's four values, cell by cell in plain Python as alignment.c:28-168 reads with is_sw = 1: slow, and nothing
    to get wrong.  A cell outside the band is never written: it keeps the 0 every cell starts with."""
    la, lb = len(a), len(b)
    W = la + 1
    go, ge = sc.gap_open + sc.gap_extend, sc.gap_extend
    M = [0] * ((lb + 1) * W)
    A = list(M)
    B = list(M)
    unknown = []
    lo, hi = (-lb, la) if band is None else band
    score, same = BL.scoring_table(sc, a, b)[:2]
    no_mm, no_end, no_ga, no_gb = bool(sc.no_mismatches), bool(sc.no_end_gap_penalty), bool(sc.no_gaps_in_a), bool(sc.no_gaps_in_b)
    for j in range(1, lb + 1):
        srow, mrow = score[b[j - 1]], same[b[j - 1]]
        for i in range(1, la + 1):
            if not lo <= i - j <= hi:
                continue
            c = j * W + i
            s = srow[a[i - 1]]
            ul, up, lf = c - W - 1, c - W, c - 1
            if s is None:
                unknown.append((i, j))
            elif no_mm and not mrow[a[i - 1]]:
                M[c] = 0
            else:
                M[c] = max(M[ul] + s, A[ul] + s, B[ul] + s, 0)
            if i == la and no_end:
                A[c] = max(M[up], A[up], B[up])
            elif (not no_ga) or i == la:
                A[c] = max(M[up] + go, A[up] + ge, B[up] + go, 0)
            else:
                A[c] = 0
            if j == lb and no_end:
                B[c] = max(M[lf], A[lf], B[lf])
            elif (not no_gb) or j == lb:
                B[c] = max(M[lf] + go, A[lf] + go, B[lf] + ge, 0)
            else:
                B[c] = 0
    as_i32 = lambda X: np.array(X, np.int64).astype(np.int32)
    return as_i32(M), as_i32(A), as_i32(B), unknown


def best_cell(M, la: int):
    """(score, end_a, end_b) of the best match_scores cell in hit order -- score descending, column ascending, index
    ascending -- 1-based; (0, 0, 0) when no cell is above 0.  What the score call returns."""
    M2 = np.asarray(M).reshape(-1, la + 1)
    best = int(M2.max())
    if best <= 0:
        return 0, 0, 0
    col = int(np.nonzero((M2 == best).any(axis=0))[0][0])
    row = int(np.nonzero(M2[:, col] == best)[0][0])
    return best, col, row


def hit_of(sc, a: bytes, b: bytes, M, A, B, min_score: int):
    """The oracle's first hit over the matrices: (rc, hit dict or None)."""
    rc, hits = O.oracle_sw_hits(sc, a, b, M, A, B, min_score, max_hits=1)
    return rc, (hits[0] if hits else None)


def expected(sc, a: bytes, b: bytes, lo: int, hi: int, min_score: int = 1):
    """((score, end_a, end_b) of the score call, the align call's hit dict or None) from one fill."""
    M, A, B = fill(sc, a, b, (lo, hi))
    rc, hit = hit_of(sc, a, b, M, A, B, min_score)
    assert rc == 0, rc
    return best_cell(M, len(a)), hit


def hit_excursion(hit):
    """(lowest, highest) i - j over the cells a hit's walk visits, its start cell (pos_a, pos_b) and its end cell included."""
    i, j = hit["pos_a"], hit["pos_b"]
    lo = hi = i - j
    for x, y in zip(hit["a"], hit["b"]):
        if x != "-":
            i += 1
        if y != "-":
            j += 1
        lo, hi = min(lo, i - j), max(hi, i - j)
    return lo, hi


def read_in_window(rng, read_len, window_len, edits: float, alphabet: bytes = b"ACGT"):
    """A read planted in a window: (seq_a = the read, seq_b = the window, offset).  The read is window[offset : offset +
    read_len] with edits at rate `edits` per letter (bandlib.mutate), so its hit lies near the diagonal i - j = -offset."""
    window = bytes(rng.choice(alphabet) for _ in range(window_len))
    offset = rng.randrange(0, max(1, window_len - read_len + 1))
    read = BL.mutate(rng, window[offset:offset + read_len], edits, alphabet)
    return read, window, offset
