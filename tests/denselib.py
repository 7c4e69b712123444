"""Gap-dense alignments for the direction-byte tests: pairs whose optimal alignment puts an insertion run directly against a
deletion run, and the scorings under which it does.  No GPU import (tests/test_dense_argument_cpu.py argues on the oracle
alone that the cases of tests/test_gpu_gap_dense.py contain what they claim; the GPU file runs the same lists).

WHY: alignment_reverse_move (src/alignment.c:311-327) tests GAP_A first, so a walk that stands in GAP_A and whose predecessor
is GAP_B -- in the gapped strings: an I run followed at once by a D run -- exists only where a mismatch costs more than one
opened gap in each sequence, mismatch < 2 (gap_open + gap_extend).  Under [1,-2,-4,-1] and [2,-2,-2,-1] it never happens.

CIGAR convention (include/seqalign_hip.h): seq_a is the query, seq_b the reference -- '-' in result_b = I, '-' in result_a = D.
"""
import random

import orclib as O

M, EQX = 1, 2

# ---------------------------------------------------------------------------------------------------------------- scorings ---
# flag-free, gap_open <= 0, gap_extend <= 0 (sa_domain_nw_dirs / sa_domain_sw_dirs); all fit int16 at 1 000 x 1 000
# (sa_domain_nw_x2_scores_fit: 2 002 x 11 = 22 022 <= 30 000 for [5,-10,0,-1], the worst of them)
SCORINGS = {
    "cheap0": {"init": [2, -9, 0, -1, 0, 0, 0, 0, 0, 0]},
    "cheap1": {"init": [2, -9, -1, -1, 0, 0, 0, 0, 0, 0]},
    "ties": {"init": [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]},            # every >= in a direction bit decides a move
    "ext0": {"init": [2, -5, -1, 0, 0, 0, 0, 0, 0, 0]},
    "swdense": {"init": [5, -10, 0, -1, 0, 0, 0, 0, 0, 0]},      # SW: under cheap0 a local hit gains nothing across 1I1D and stays 1M
    "cheap0N": {"init": [2, -9, 0, -1, 0, 0, 0, 0, 0, 0], "wildcards": [["N", 0]]},   # the LDS-table instantiations
}
NW_SCORINGS = tuple(SCORINGS)
SW_SCORINGS = ("swdense", "ties", "ext0")
CONTROLS = {"default": {"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]}, "sw_default": {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}}

_OSC = {}


def oracle_scoring(name):
    if name not in _OSC:
        _OSC[name] = O.build_scoring({**SCORINGS, **CONTROLS}[name], "oracle")
    return _OSC[name]


# ------------------------------------------------------------------------------------------------------------------ helpers ---
def ops(ra, rb) -> str:
    """One letter per column of the gapped strings: M, I ('-' in result_b) or D ('-' in result_a)."""
    if isinstance(ra, str):
        ra, rb = ra.encode(), rb.encode()
    assert len(ra) == len(rb)
    return "".join("D" if x == 45 else "I" if y == 45 else "M" for x, y in zip(ra, rb))


def count_id(ra, rb) -> int:
    """Insertion runs followed at once by a deletion run."""
    return ops(ra, rb).count("ID")


def count_di(ra, rb) -> int:
    """Deletion runs followed at once by an insertion run (alignment_reverse_move never produces one on a flag-free scoring)."""
    return ops(ra, rb).count("DI")


def cigar(ra, rb, fmt=M, fold=True) -> str:
    """include/seqalign_hip.h's definition once more, independent of both C encoders."""
    if isinstance(ra, str):
        ra, rb = ra.encode(), rb.encode()
    runs = []
    for x, y in zip(ra, rb):
        if x == 45: op = "D"
        elif y == 45: op = "I"
        elif fmt == M: op = "M"
        else: op = "=" if (bytes([x]).lower() == bytes([y]).lower() if fold else x == y) else "X"
        if runs and runs[-1][0] == op: runs[-1][1] += 1
        else: runs.append([op, 1])
    return "".join(f"{n}{op}" for op, n in runs)


# ------------------------------------------------------------------------------------------------------------- pair families ---
LETTERS = [(x, y, z) for x in b"ACGT" for y in b"ACGT" for z in b"ACGT" if len({x, y, z}) == 3]     # 24 triples


def _triple(k: int):
    return LETTERS[(7 * k) % len(LETTERS)]


def matches_of(scoring: str) -> int:
    """Matching letters per period of the alternating stretches.  One -- (xy)^m against (xz)^m, 1M1I1D, 3 steps per period --
    except under ext0: with gap_extend 0 a single match between two substitutions only TIES one long deletion run plus one long
    insertion run over all of them, and the reference takes the long runs (one I->D per stretch); three matches per period
    (3M1I1D, 5 steps) make the separate 1I1D strictly better.  3 and 5 are both coprime to 32, 64, 8 and 16."""
    return 3 if scoring == "ext0" else 1


def _units(k: int, matches: int):
    x, y, z = _triple(k)
    w = [c for c in b"ACGT" if c not in (x, y, z)][0]
    same = bytes([x, w, x][:matches])
    return same + bytes([y]), same + bytes([z]), (x, y, z, w)


def alternation(la: int, lb: int, k: int = 0, matches: int = 1):
    """a = (xy)^m + T, b = (xz)^m + T cut to la and lb letters, T a tail of k % 6 matching letters: under a cheap-gap scoring
    1M1I1D per period -- 3 steps, coprime to 32, 64, 8 and 16, so that a walk of >= 192 steps puts the GAP_A-from-GAP_B
    transition on every position of a 32-column move word, a 64-byte tile edge and an 8 x 16 direction block.  k picks the three
    letters and the tail: pairs of ONE shape that differ.  matches: matching letters per period (matches_of)."""
    ua, ub, (x, y, z, w) = _units(k, matches)
    t = min(k % 6, la, lb)
    tail = bytes([w, x, w, w, y, w][:t])
    a = (ua * (la // len(ua) + 1))[:la - t] + tail
    b = (ub * (lb // len(ub) + 1))[:lb - t] + tail
    return a, b


def spaced(la: int, lb: int, seed: int, k: int = 0, twice: bool = False, matches: int = 1):
    """Alternating stretches of 1 .. 6 periods separated by matching spacers of 1 .. 12 random letters, cut to la and lb: long
    match bursts and single transitions mix.  The structure comes from `seed`, the stretches' letters from k (pairs of one
    shape that differ).  twice: the first half planted again behind a short unrelated piece, so that several local hits share
    cells (the SW multi-hit cases)."""
    rng = random.Random(seed)
    ua, ub, (x, y, z, w) = _units(k, matches)
    a, b = bytearray(), bytearray()
    need = max(la, lb) if not twice else (max(la, lb) - 6) // 2
    while len(a) < need:
        n = rng.randint(1, 6)
        a += ua * n
        b += ub * n
        sp = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 12)))
        a += sp
        b += sp
    if twice:
        a, b = a[:need], b[:need]
        a = a + bytes([y]) * 3 + a
        b = b + bytes([z]) * 6 + b
    return bytes(a[:la]), bytes(b[:lb])


def substituted(la: int, lb: int, seed: int):
    """b = a slice of a with 20 % substitutions: each isolated substitution becomes 1I1D under a cheap-gap scoring.  Only ever
    ADDED to batches -- at short or lopsided shapes some pairs have no I->D at all -- never counted towards a guarantee."""
    rng = random.Random(seed)
    a = bytes(rng.choice(b"ACGT") for _ in range(la))
    o = rng.randint(0, max(0, la - lb))
    b = bytearray((a[o:] + bytes(rng.choice(b"ACGT") for _ in range(lb)))[:lb])
    for i in range(len(b)):
        if rng.random() < 0.2:
            b[i] = rng.choice([c for c in b"ACGT" if c != b[i]])
    return a, bytes(b)


def long_runs(k: int = 0):
    """a = X + P + Y, b = X + Q + Y, P and Q 200 letters from disjoint alphabets: an insertion run and a deletion run of ~200
    columns each, back to back -- the transition sits at the end of runs that cross several tiles in a gap state.  Where the
    runs meet depends on chance matches of Y's first letters (60M200I1D1M199D59M, 60M200I200D60M, ...); that they meet, and
    that both are >= 198 long, is pinned in test_dense_argument_cpu.py."""
    rng = random.Random(4000 + k)
    X = bytes(rng.choice(b"ACGT") for _ in range(60))
    Y = bytes(rng.choice(b"ACGT") for _ in range(60))
    P = bytes(rng.choice(b"AC") for _ in range(200))
    Q = bytes(rng.choice(b"GT") for _ in range(200))
    return X + P + Y, X + Q + Y


def long_run_pairs():
    """The long-runs and staircase pairs of the walker cases (seed 2: a chance match of Y[0] keeps the two runs a column apart)."""
    return [long_runs(k) for k in (1, 3, 4)] + [staircase(100, 77), staircase(64, 64), staircase(33, 191)]


def staircase(la: int, lb: int):
    """Disjoint alphabets: two runs, la + lb columns."""
    return (b"AC" * la)[:la], (b"GT" * lb)[:lb]


# ----------------------------------------------------------------------------------------------------------------- the cases ---
# NW shapes: name -> (len_a, len_b, pairs per batch, the I->D transitions EVERY counted pair of the shape has under every scoring
# of NW_SCORINGS -- checked pair by pair in test_dense_argument_cpu.py).
#   150x150, 31x40, 191x150: rows of <= 192 columns, the four-per-wave fills' domain;  31 x 40 holds at most 15 periods and its
#   spaced pairs fewer: its floor is 3, every other shape's is 8
#   m250: 501 columns, 8 per lane;  m500 and wide (m_a = 500 against m_b = 45): 1 001 columns, 16 per lane -- the direction fill
#   takes such rows from 384 pairs up (sa_host::nw_dirs_applicable), so those batches repeat a few distinct pairs
NW_SHAPES = {
    "150x150": (150, 150, 37, 8),
    "31x40": (31, 40, 37, 3),
    "191x150": (191, 150, 37, 8),
    "m250": (500, 500, 37, 8),
    "m500": (1000, 1000, 384, 8),
    "wide": (1000, 90, 384, 8),
}
QUAD_SHAPES = ("150x150", "31x40", "191x150")      # rows of <= 192 columns
DISTINCT_WIDE = 8                                  # distinct pairs in the 384-pair batches


def nw_alternation(shape: str, scoring: str):
    """The distinct alternation pairs of the shape."""
    la, lb, n, _ = NW_SHAPES[shape]
    return [alternation(la, lb, k, matches_of(scoring)) for k in range(min(n, 24) if n < 100 else DISTINCT_WIDE)]


def nw_uniform(shape: str, scoring: str):
    """Pairs all of the shape -- what the packed fills take two / four per wave: alternation and, every third one, spaced
    (wide: alternation only, see nw_ragged)."""
    la, lb, n, _ = NW_SHAPES[shape]
    m = matches_of(scoring)
    d = n if n < 100 else DISTINCT_WIDE
    distinct = [spaced(la, lb, 17 * la + k, k, matches=m) if k % 3 == 2 and shape != "wide" else alternation(la, lb, k, m) for k in range(d)]
    return [distinct[p % d] for p in range(n)]


def _ragged_lengths(la, lb, rng):
    cut = (lambda v: v - rng.randint(0, min(6, v // 8)))
    return cut(la), cut(lb)


def nw_ragged(shape: str, scoring: str):
    """Spaced and alternation pairs of many lengths up to the shape, every structure twice with different letters so that the
    bucketed fill finds partners.  (wide: alternation only -- a spaced seq_b of 90 letters finds better places along a
    repetitive seq_a of 1 000 than the planted one.)"""
    la, lb, n, _ = NW_SHAPES[shape]
    m = matches_of(scoring)
    rng = random.Random(la * 1009 + lb)
    d = (n if n < 100 else 2 * DISTINCT_WIDE) - 1
    distinct = []
    for q in range(d // 2):
        xa, xb = _ragged_lengths(la, lb, rng)
        if q % 3 == 2 or shape == "wide":
            distinct += [alternation(xa, xb, q, m), alternation(xa, xb, q + 5, m)]
        else:
            distinct += [spaced(xa, xb, la + 31 * q, q, matches=m), spaced(xa, xb, la + 31 * q, q + 5, matches=m)]
    distinct.append(alternation(la, lb, 3, m) if shape == "wide" else spaced(la, lb, la + 7, 3, matches=m))
    return [distinct[p % len(distinct)] for p in range(n)]


def nw_extra(shape: str, scoring: str):
    """Substituted pairs of the shape -- with the wildcard scoring some letters are N -- added to batches, never counted."""
    la, lb, n, _ = NW_SHAPES[shape]
    out = [substituted(la, lb, seed=la + lb + s) for s in range(4 if n < 100 else 2)]
    if scoring == "cheap0N":
        rng = random.Random(la)
        out = [tuple(bytes(78 if rng.random() < 0.05 else c for c in s) for s in pair) for pair in out]
    return out


def nw_mostly_one_shape(shape: str, scoring: str):
    """Three quarters of the pairs of ONE shape (alternation), the rest ragged: both kinds of waves in one grid."""
    uni, rag = nw_uniform(shape, scoring), nw_ragged(shape, scoring)
    return [rag[p] if p % 4 == 3 else uni[p] for p in range(len(uni))]


def walker_pairs(shape: str, scoring: str, n: int = 37):
    """The walker axes' batch: alternation and spaced pairs, half of them ragged."""
    la, lb = NW_SHAPES[shape][:2]
    m = matches_of(scoring)
    rng = random.Random(la + 5)
    out = []
    for q in range(n):
        xa, xb = _ragged_lengths(la, lb, rng) if q % 2 else (la, lb)
        out.append(alternation(xa, xb, q, m) if q % 3 == 0 else spaced(xa, xb, 3 * la + q, q, matches=m))
    return out


# SW: the same families; the best hit of an alternation pair is the whole pair (CIGARs of 2 x 223 bytes at 150 x 150)
SW_SHAPES = {"150x150": (150, 150, 37, 8), "31x40": (31, 40, 37, 3), "191x150": (191, 150, 37, 8), "m250": (500, 500, 9, 8)}
SW_MIN_SCORE = 4


def sw_uniform(shape: str, scoring: str):
    la, lb, n, _ = SW_SHAPES[shape]
    m = matches_of(scoring)
    # (31 x 40: alternation only -- a spaced pair that short can hold a single stretch of one period)
    return [alternation(la, lb, k, m) if k % 2 or shape == "31x40" else spaced(la, lb, 9 * la + k // 2, k, matches=m) for k in range(n)]


def sw_ragged(shape: str, scoring: str):
    la, lb, n, _ = SW_SHAPES[shape]
    m = matches_of(scoring)
    rng = random.Random(la * 2003 + lb)
    out = []
    for q in range(n // 2):
        xa, xb = _ragged_lengths(la, lb, rng)
        if shape == "31x40":
            out += [alternation(xa, xb, q, m), alternation(xa, xb, q + 5, m)]
        else:
            out += [spaced(xa, xb, 5 * la + q, q, matches=m), spaced(xa, xb, 5 * la + q, q + 5, matches=m)]
    out.append(alternation(la, lb, 1, m))
    return out


def sw_planted_twice(scoring: str, n: int = 21, la: int = 150, lb: int = 160):
    """Spaced alternation with the stretch planted twice: several dense hits share cells, and the visited mask cuts walks."""
    return [spaced(la - q % 5, lb - q % 3, 700 + q, q, twice=True, matches=matches_of(scoring)) for q in range(n)]


def counted_nw_cases(scoring: str):
    """(label, floor, pairs): every list of pairs a GPU NW case counts on, for the argument file."""
    for shape, (_, _, _, floor) in NW_SHAPES.items():
        yield "uniform:" + shape, floor, nw_uniform(shape, scoring)
        yield "ragged:" + shape, floor, nw_ragged(shape, scoring)
    for shape in ("150x150", "m250"):
        yield "walkers:" + shape, 8, walker_pairs(shape, scoring)


def counted_sw_cases(scoring: str):
    for shape, (_, _, _, floor) in SW_SHAPES.items():
        yield "uniform:" + shape, floor, sw_uniform(shape, scoring)
        yield "ragged:" + shape, floor, sw_ragged(shape, scoring)
    yield "planted-twice", 8, sw_planted_twice(scoring)


# ------------------------------------------------------------------------------------- the span, band and long-SW cases ---
# tests/test_gpu_sw_span_dense.py and tests/test_gpu_band_dense.py run these lists; tests/test_span_band_dense_argument_cpu.py
# argues on the oracle alone that they contain what those files claim.
SPAN_STRIP_COLS = 512
# (len_a, len_b), one per class of the span launcher: 1, 2, 3, 3, 4, 5, 6 and 8 columns per lane, and a pair of 1 100 rows (many
# 64-row code fetches) ...
SPAN_ROWS_SHAPES = ((60, 60), (100, 90), (130, 90), (190, 150), (250, 120), (320, 100), (384, 100), (512, 100), (150, 1100))
# ... and rows of two to five strips; the last three run through several hand-off blocks of 64 rows
SPAN_STRIPS_SHAPES = ((513, 150), (577, 129), (700, 64), (1100, 150), (1600, 90), (1100, 1100), (1600, 700), (2100, 300))
SPAN_K = range(8)


def straddling(la: int, lb: int, k: int = 0, matches: int = 1, seam: int = SPAN_STRIP_COLS):
    """alternation's two stretches, min(la, lb) letters each and without the tail; seq_a's stands in la letters of y -- which
    seq_b lacks -- with column `seam` in its middle (as far as la lets it): the dense hit crosses the seam wherever
    alternation's own sits left or right of it."""
    ua, ub, (x, y, z, w) = _units(k, matches)
    n = min(la, lb)
    at = max(0, min(la - n, seam - n // 2))
    a = bytes([y]) * at + (ua * (n // len(ua) + 1))[:n] + bytes([y]) * (la - at - n)
    return a, (ub * (lb // len(ub) + 1))[:lb]


def span_counted(la: int, lb: int, scoring: str):
    """The counted pairs of one span shape: alternation, k = 0 .. 7."""
    return [alternation(la, lb, k, matches_of(scoring)) for k in SPAN_K]


def span_seam(la: int, lb: int, scoring: str):
    """The seam pairs of a shape of several strips: straddling, k = 0 .. 7, where the stretch can be centred on column 512
    (not at 513 x 150: there alternation's own hits reach the last column, 513)."""
    if la <= SPAN_STRIP_COLS or la - min(la, lb) < SPAN_STRIP_COLS - min(la, lb) // 2:
        return []
    return [straddling(la, lb, k, matches_of(scoring)) for k in SPAN_K]


def span_added(la: int, lb: int, scoring: str):
    """Spaced pairs of the shape: added to the calls, never counted."""
    return [spaced(la, lb, 23 * la + lb + k, k, matches=matches_of(scoring)) for k in (1, 4)]


# banded SW: (len_a, len_b) of the alternation pairs, k = 0 .. 5, and the bands (diag_lo, diag_hi) of each
BAND_SHAPES = ((150, 150), (191, 150), (500, 500))
BAND_K = range(6)


def sw_bands(la: int, lb: int):
    """The whole matrix; the excursion of the unbanded hit and one diagonal more; exactly it, (0, +1): I->D; its mirror
    (-1, 0): the same score through D->I only; the main diagonal alone; a wide band; a band the hit's diagonals lie outside."""
    return [(-lb, la), (-1, 1), (0, 1), (-1, 0), (0, 0), (-40, 40), (30, 60)]


def band_pairs(la: int, lb: int, scoring: str):
    return [alternation(la, lb, k, matches_of(scoring)) for k in BAND_K]


def band_added(la: int, lb: int, scoring: str):
    """Spaced pairs of the shape, added to the band calls: alternation's period is two columns (three steps), so its
    transitions stand in every second column only; the spacers shift the stretches onto every column of a strip of 64."""
    return [spaced(la, lb, 13 * la + k, k, matches=matches_of(scoring)) for k in (1, 4)]


# past the narrow calls' cap of 1 024 diagonals: one pair, SW under swdense within (-600, 600), NW under cheap0 with band 600
PAST_CAP = dict(shape=(1300, 1300), sw=("swdense", -600, 600), nw=("cheap0", 600))


def long_sw_pairs():
    """test_nw_align_long_seams_inside_alternating_stretches's pairs and one of three strips' width."""
    return [alternation(150, 150, 0), alternation(191, 150, 4), alternation(500, 500, 1), spaced(300, 260, 11, 2),
            spaced(150, 150, 12, 3), alternation(31, 40, 5)] + long_run_pairs()[:2] + [alternation(1100, 300)]
