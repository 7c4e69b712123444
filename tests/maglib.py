"""Large score magnitudes: scorings multiplied by a scale, the small pairs they run on, and an exact-integer restatement of
the three-matrix recurrence that says how far the values go.  No GPU import (tests/test_magnitude_argument_cpu.py argues on
the oracle alone that the cases of tests/test_gpu_magnitude.py are what they claim; the GPU file runs the same lists).

WHY: every other test draws a match of 1 .. 6 and penalties no lower than -13, so no int32 kernel ever saw a cell above a few
tens of thousands.  The recurrence is positively homogeneous -- multiply every number of the scoring by s > 0 and every value
that does not come from the NW floor is multiplied by s -- so one small pair reaches any magnitude: the scale is chosen per
(family, shape, NW | SW) from the largest cell of the shape's pairs at scale 1.  A kernel that de-trends gap_b (sa_rowsweep.hpp: w(g) = cin(g) + g |gap_extend|) forms
sums the reference never forms; `admitted` below is the library's documented rule for them, restated.

CIGAR / gap naming as the reference's: gap_b_scores moves ALONG a row (a letter of seq_a against '-' in result_b), gap_a_scores
down a column ('-' in result_a).
"""
from __future__ import annotations

import random

import numpy as np

import orclib as O

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
FRAME_COLS, FILL_FRAME_COLS = 1024, 4096     # the widest frames the kernels de-trend over (include/seqalign_hip.h, SEQALIGN_E_DOMAIN)

# ------------------------------------------------------------------------------------------------------------ scorings ---
# base profiles at scale 1: init = match, mismatch, gap_open, gap_extend, no_start, no_end, no_gaps_in_a, no_gaps_in_b,
# no_mismatches, case_sensitive.  All inside the NW parity domain (no penalty below -|min_penalty|).
BASES = {
    "dna": {"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]},
    "open0": {"init": [2, -3, 0, -1, 0, 0, 0, 0, 0, 0]},
    "extpos": {"init": [3, -2, -5, 1, 0, 0, 0, 0, 0, 0]},           # a gap that pays from its second column on
    "nostart": {"init": [1, -2, -4, -1, 1, 0, 0, 0, 0, 0]},
    "noend": {"init": [1, -2, -4, -1, 0, 1, 0, 0, 0, 0]},
    "nogaps_a": {"init": [1, -2, -4, -1, 0, 0, 1, 0, 0, 0]},
    "nogaps_b": {"init": [1, -2, -4, -1, 0, 0, 0, 1, 0, 0]},
    "nomismatch": {"init": [2, -2, -3, -1, 0, 0, 0, 0, 1, 0]},
    # a table with asymmetric entries: (a, c) != (c, a), a match that scores above `match`, a mismatch that pays
    "mut": {"init": [1, -3, -4, -1, 0, 0, 0, 0, 0, 0],
            "mutations": [["a", "c", -1], ["c", "a", -3], ["g", "t", 2], ["t", "g", -2], ["a", "a", 3]]},
    # at the floor: the named penalty EQUALS -|min_penalty|, so floor + penalty == INT32_MIN, and the flag leaves floor cells
    "floor_a": {"init": [3, -5, -4, -1, 0, 0, 1, 0, 0, 0]},         # mismatch = open1 = -5; gap_a at the floor inside
    "floor_b": {"init": [3, -5, -4, -1, 0, 0, 0, 1, 0, 0]},         # ... gap_b at the floor above the last row
    "floor_mm": {"init": [2, -6, -5, -1, 0, 0, 0, 0, 1, 0]},        # open1 = -6 against blocked match cells
    # top: a match far above the gap penalties, so that a pair's peak can stand near 2^31 with room for the de-trend ...
    "steep": {"init": [64, -48, -5, -1, 0, 0, 0, 0, 0, 0]},
    # ... and one where it cannot: match = -gap_extend = -mismatch (the case sa_rowsweep.hpp's high side was found on)
    "flat": {"init": [1, -1, 0, -1, 0, 0, 0, 0, 0, 0]},
}
FLOOR_BASES = ("floor_a", "floor_b", "floor_mm")
POWERS = (15, 16, 23, 24, 27)
TOP = "top"
DEEP = "deep"
DEEP_PEAK = 18 * 2 ** 30 // 10      # 1.8 * 2^30
DEEP_BASES = ("dna", "flat", "mut", "floor_a")
# (base, what the peak crosses): a power of two p -- the peak lands in [2^p, 2^(p + 1)) -- or TOP: in [2^30, 2^31) -- or DEEP:
# the largest scale at which it stays at or below 1.8 * 2^30.  TOP takes the SMALLEST scale that reaches 2^30, and on these pairs
# the peak is a positive cell or a border cell, so no real NW score lies below -2^30 there; under DEEP the long pairs' global
# scores and banded end values stand in (-2^31, -2^30): real scores below INT32_MIN / 2, far above the floor (NW only; not
# nomismatch / floor_mm, whose align walker steps along the floor and muddies what "has an alignment" means)
FAMILIES = tuple(("dna", p) for p in POWERS) + (
    ("open0", 16), ("extpos", 23), ("nostart", 15), ("noend", 24), ("nogaps_a", 24), ("nogaps_b", 27), ("nomismatch", 16),
    ("mut", 23), ("floor_a", 29), ("floor_b", 29), ("floor_mm", 29), ("steep", TOP), ("flat", TOP), ("extpos", TOP)) + tuple(
    (base, DEEP) for base in DEEP_BASES)


def nw_only(fam) -> bool:
    """The families that run under NW alone: the floor families (under SW the floor is the score 0) and the deep ones (their
    magnitude is a NW score's; SW has no negative cell)."""
    return fam[0] in FLOOR_BASES or fam[1] == DEEP


def family_id(fam) -> str:
    return f"{fam[0]}@{fam[1]}"


def scaled(spec: dict, s: int) -> dict:
    """Every number of the scoring times s."""
    out = {"init": [v * s for v in spec["init"][:4]] + list(spec["init"][4:])}
    if "mutations" in spec:
        out["mutations"] = [[x, y, v * s] for x, y, v in spec["mutations"]]
    return out


def numbers(spec: dict):
    return list(spec["init"][:4]) + [v for _, _, v in spec.get("mutations", [])]


def min_penalty(spec: dict) -> int:
    """scoring_init / scoring_add_mutation (alignment_scoring.c:49-54, :70)."""
    m, mm, go, ge = spec["init"][:4]
    lo = min(m, mm)
    if not (spec["init"][6] and spec["init"][7]):
        lo = min(lo, go + ge, ge)
    return min([lo] + [v for _, _, v in spec.get("mutations", [])])


_OSC = {}


def oracle_scoring(spec: dict):
    key = repr(spec)
    if key not in _OSC:
        _OSC[key] = O.build_scoring(spec, "oracle")
    return _OSC[key]


def lookup(spec: dict):
    """scoring_lookup (alignment_scoring.c:133-176) for a scoring without wildcards, as a function of two letters: the score,
    or None where no_mismatches blocks the pair."""
    m, mm = spec["init"][:2]
    no_mm, case = bool(spec["init"][8]), bool(spec["init"][9])
    table = {(ord(x), ord(y)): v for x, y, v in spec.get("mutations", [])}
    fold = (lambda c: c) if case else (lambda c: c + 32 if 65 <= c <= 90 else c)

    def score(x: int, y: int):
        x, y = fold(x), fold(y)
        if no_mm and x != y:
            return None
        if (x, y) in table:
            return table[(x, y)]
        return m if x == y else mm
    return score


# ------------------------------------------------------------------------------------------------- the exact reference ---
class Exact:
    """What exact_fill returns: M, A, B as lists of Python ints (pitch len_a + 1); lo / hi: the smallest and the largest result
    of any add or multiply the reference's C performs (alignment.c:38-155), floor + penalty included; peak: the largest |value|
    among those that do not descend from the NW floor, border cells included; floor: alignment.c:41's min."""
    __slots__ = ("M", "A", "B", "lo", "hi", "peak", "top", "floor")

    def fits_int32(self) -> bool:
        return INT32_MIN <= self.lo and self.hi <= INT32_MAX


def exact_fill(spec: dict, a: bytes, b: bytes, is_sw: int) -> Exact:
    """alignment_fill_matrices (alignment.c:28-168) in Python ints, nothing wraps.  Beside every value goes one bit: it descends
    from the floor constant (NW only: under SW the floor is the score 0).  The maximum of values keeps the bit of the winner."""
    la, lb = len(a), len(b)
    W = la + 1
    m_, mm_, go_, ge = spec["init"][:4]
    no_start, no_end, no_ga, no_gb = (bool(v) for v in spec["init"][4:8])
    look = lookup(spec)
    sums = [go_ + ge]                       # every result of C arithmetic that is not formed cell by cell below
    open1 = go_ + ge
    mn = 0 if is_sw else INT32_MIN + abs(min_penalty(spec))
    fl = not is_sw                          # the floor's bit
    n = W * (lb + 1)
    M, A, B = [mn] * n, [mn] * n, [mn] * n
    TM, TA, TB = [fl] * n, [fl] * n, [fl] * n
    M[0] = A[0] = B[0] = 0
    TM[0] = TA[0] = TB[0] = False
    if is_sw:
        for i in range(1, W):
            TM[i] = TA[i] = TB[i] = False
    else:
        for i in range(1, W):
            if no_start:
                B[i] = 0
            else:
                sums += [i * ge, go_ + i * ge]
                B[i] = go_ + i * ge
            TB[i] = False
        for j in range(1, lb + 1):
            if no_start:
                A[j * W] = 0
            else:
                sums += [j * ge, go_ + j * ge]
                A[j * W] = go_ + j * ge
            TA[j * W] = False
    lo, hi = min(sums), max(sums)
    peak = max(abs(v) for v in sums)
    top = max(sums + [0])

    def best(c):
        # the largest value; among equal values one that does not descend from the floor
        v = max(c)[0]
        return v, (v, False) not in c

    for j in range(1, lb + 1):
        y = b[j - 1]
        last_row = j == lb
        for i in range(1, W):
            c = j * W + i
            ul, up, lf = c - W - 1, c - W, c - 1
            last_col = i == la
            s = look(a[i - 1], y)
            # each entry: (value, descends from the floor); `adds` collects what C computed, `real` what of it counts as peak
            if s is None:
                cm = (mn, fl)
                adds = []
            else:
                adds = [(M[ul] + s, TM[ul]), (A[ul] + s, TA[ul]), (B[ul] + s, TB[ul])]
                cm = best(adds + [(mn, fl)])
            if last_col and no_end:
                ca = best([(M[up], TM[up]), (A[up], TA[up]), (B[up], TB[up])])
            elif not no_ga or last_col:
                t = [(M[up] + open1, TM[up]), (A[up] + ge, TA[up]), (B[up] + open1, TB[up])]
                adds += t
                ca = best(t + [(mn, fl)])
            else:
                ca = (mn, fl)
            if last_row and no_end:
                cb = best([(M[lf], TM[lf]), (A[lf], TA[lf]), (B[lf], TB[lf])])
            elif not no_gb or last_row:
                t = [(M[lf] + open1, TM[lf]), (A[lf] + open1, TA[lf]), (B[lf] + ge, TB[lf])]
                adds += t
                cb = best(t + [(mn, fl)])
            else:
                cb = (mn, fl)
            for v, t in adds:
                if v < lo: lo = v
                if v > hi: hi = v
                if not t:
                    if v > top: top = v
                    if v > peak: peak = v
                    elif -v > peak: peak = -v
            M[c], TM[c] = cm
            A[c], TA[c] = ca
            B[c], TB[c] = cb
    out = Exact()
    out.M, out.A, out.B, out.lo, out.hi, out.peak, out.top, out.floor = M, A, B, lo, hi, peak, top, mn
    return out


def cells_peak(M, A, B) -> int:
    """The largest |value| of the oracle's matrices AT SCALE 1, where anything below -2^30 descends from the floor."""
    peak = 0
    for X in (M, A, B):
        X = np.asarray(X, np.int64)
        real = X[X > -2 ** 30]
        if real.size:
            peak = max(peak, int(np.abs(real).max()))
    return peak


# --------------------------------------------------------------------------------------------------------------- pairs ---
# (name, len_a, len_b): 41 columns = 1 per lane; 97 = 2 per lane, and square, so that a band can cut a path; 501 = 8; 1 001 =
# 16; 1 101 = the strips forms of the score-family calls.  The planted pairs' len_a is one off.
SHAPES = (("c1", 40, 24), ("sq", 96, 96), ("c8", 500, 24), ("c16", 1000, 24), ("strips", 1100, 24))
KINDS = ("ident", "disjoint", "gapb", "gapa")
PLANT = 20          # columns between the planted gap and the end


def _letters(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def _other(*avoid):
    return [c for c in b"ACGT" if c not in avoid][0]


def pair(shape: str, kind: str):
    """(seq_a, seq_b).  T = len_b random letters; seq_a ends with T (ident), with T and one letter x more PLANT columns before
    the end (gapb: the path opens a gap_b right after the row's highest cells), with T less one letter (gapa); F fills seq_a
    up to about len_a in front.  disjoint: seq_a over AC, seq_b over GT.  `both` (square only): one gap each way, 35 columns
    apart -- the path leaves the main diagonal and comes back."""
    name, la, lb = next(s for s in SHAPES if s[0] == shape)
    rng = random.Random(f"{shape}/{kind}")
    T = _letters(rng, lb)
    k = min(PLANT, lb // 2)
    if kind == "disjoint":
        return _letters(rng, la, b"AC"), _letters(rng, lb, b"GT")
    if kind == "ident":
        return _letters(rng, la - lb) + T, T
    if kind == "gapb":
        x = _other(T[lb - k - 1], T[lb - k])
        return _letters(rng, max(0, la - lb - 1)) + T[:lb - k] + bytes([x]) + T[lb - k:], T
    if kind == "gapa":
        while T[lb - k] in (T[lb - k - 1], T[lb - k + 1]):          # the deleted letter differs from both neighbours
            T = T[:lb - k] + bytes([_other(T[lb - k - 1], T[lb - k + 1])]) + T[lb - k + 1:]
        return _letters(rng, max(0, la - lb + 1)) + T[:lb - k] + T[lb - k + 1:], T
    if kind == "both":
        assert la == lb
        x = _other(T[39], T[40])
        if T[75] in (T[74], T[76]):
            T = T[:75] + bytes([_other(T[74], T[76])]) + T[76:]
        return T[:40] + bytes([x]) + T[40:75] + T[76:], T
    raise KeyError(kind)


def planted(shape: str, kind: str):
    """Where the planted gap stands: ('b', i) -- seq_a's letter i (1-based) faces '-' in result_b -- or ('a', j)."""
    a, b = pair(shape, kind)
    k = min(PLANT, len(b) // 2)
    if kind == "gapb":
        return [("b", len(a) - k)]
    if kind == "gapa":
        return [("a", len(b) - k + 1)]
    if kind == "both":
        return [("b", 41), ("a", 76)]
    return []


def gaps_of(ra, rb):
    """{('b', i)} | {('a', j)} of an alignment's gapped strings: seq_a's letter i (1-based within the strings) faces '-', or
    seq_b's letter j does."""
    if isinstance(ra, str):
        ra, rb = ra.encode(), rb.encode()
    out, i, j = set(), 0, 0
    for x, y in zip(ra, rb):
        i += x != 45
        j += y != 45
        if y == 45:
            out.add(("b", i))
        if x == 45:
            out.add(("a", j))
    return out


LOOSE_A = ("open0", "mut", "steep", "flat", "noend")


def argued(base: str, kind: str, bands: bool = False) -> bool:
    """Whether tests/test_magnitude_argument_cpu.py argues that the oracle's alignment passes through the pair's planted gaps
    (bands: that the band lists hold or cut it).  Not under extpos and the floor profiles, whose alignments put gaps wherever
    gaps pay; not where no_gaps_in_a / no_gaps_in_b forbids a planted gap; not for gapa under LOOSE_A, where gaps are cheap
    against a match and a long seq_a offers better places; not for bands under no_end_gap_penalty, whose free end gaps move
    the path."""
    f = BASES[base]["init"]
    if kind not in ("gapb", "gapa", "both") or base == "extpos" or base in FLOOR_BASES:
        return False
    if (kind == "gapa" and base in LOOSE_A) or (bands and base == "noend"):
        return False
    need = {"gapb": "b", "gapa": "a", "both": "ab"}[kind]
    return not (("a" in need and f[6]) or ("b" in need and f[7]))


# ---------------------------------------------------------------------------------------------------------------- cases ---
class Case:
    """One (family, shape, NW | SW, kind): the pair, and the scoring scaled for the (family, shape, NW | SW) GROUP -- every
    kind of a group runs under one scoring, so a group is one batch."""

    def __init__(self, fam, shape, kind, is_sw, scale):
        self.fam, self.shape, self.kind, self.is_sw, self.scale = fam, shape, kind, is_sw, scale
        self.spec = scaled(BASES[fam[0]], scale)
        self.a, self.b = pair(shape, kind)

    @property
    def group(self):
        return (self.fam, self.shape, self.is_sw)

    @property
    def id(self):
        return f"{family_id(self.fam)}-{self.shape}-{'sw' if self.is_sw else 'nw'}-{self.kind}"

    def osc(self):
        return oracle_scoring(self.spec)


_BASE_PEAK = {}


def kinds_of(shape: str):
    return KINDS + (("both",) if shape == "sq" else ())


def base_peak(base: str, shape: str, is_sw: int) -> int:
    """The largest |cell| over the shape's pairs at scale 1, from the oracle."""
    key = (base, shape, is_sw)
    if key not in _BASE_PEAK:
        peak = 1
        for kind in kinds_of(shape):
            a, b = pair(shape, kind)
            rc, M, A, B = O.oracle_fill(oracle_scoring(BASES[base]), a, b, is_sw)
            assert rc == 0
            peak = max(peak, cells_peak(M, A, B))
        _BASE_PEAK[key] = peak
    return _BASE_PEAK[key]


def scale_for(fam, shape: str, is_sw: int) -> int:
    """The smallest scale (+ 1 for the powers: the low bits are populated too) at which the largest cell of the shape's pairs
    reaches 2^p (TOP: 2^30); DEEP: the largest at which it stays at or below 1.8 * 2^30."""
    base, what = fam
    bp = base_peak(base, shape, is_sw)
    if what == DEEP:
        return DEEP_PEAK // bp
    return -(-2 ** 30 // bp) if what == TOP else -(-2 ** what // bp) + 1


_CASES = None


def cases():
    """Every case of the matrix.  The floor and the deep families are NW only (nw_only)."""
    global _CASES
    if _CASES is None:
        _CASES = [Case(fam, shape, kind, is_sw, scale_for(fam, shape, is_sw))
                  for fam in FAMILIES for shape, _, _ in SHAPES for is_sw in (0, 1) if not (is_sw and nw_only(fam))
                  for kind in kinds_of(shape)]
    return _CASES


def cases_of(fam=None, shape=None, is_sw=None, kind=None):
    return [c for c in cases() if (fam is None or c.fam == fam) and (shape is None or c.shape == shape)
            and (is_sw is None or c.is_sw == is_sw) and (kind is None or c.kind == kind)]


def groups(fam=None, is_sw=None):
    """[(fam, shape, is_sw, cases of the group)] in matrix order."""
    out = {}
    for c in cases_of(fam=fam, is_sw=is_sw):
        out.setdefault(c.group, []).append(c)
    return [(*g, cs) for g, cs in out.items()]


def group_lengths(cs):
    return max(len(c.a) for c in cs), max(len(c.b) for c in cs)


_EXACT = {}


def exact(case: Case) -> Exact:
    if case.id not in _EXACT:
        _EXACT[case.id] = exact_fill(case.spec, case.a, case.b, case.is_sw)
    return _EXACT[case.id]


# ------------------------------------------------------------------------------------------------- the admission rule ---
def value_bound(spec: dict, la: int, lb: int) -> int:
    """include/seqalign_hip.h, SEQALIGN_E_DOMAIN: no cell of a pair of up to la x lb letters holds more than the best of
    m P + (la + lb - 2 m) G over m = 0 and m = min(la, lb) aligned letter pairs; P = the largest substitution score above 0,
    G = the largest of gap_open + gap_extend and gap_extend above 0."""
    m, mm, go, ge = spec["init"][:4]
    P = max([0, m] + ([] if spec["init"][8] else [mm]) + [v for _, _, v in spec.get("mutations", [])])
    G = max(0, go + ge, ge)
    n = min(la, lb)
    return max(n * P + (la + lb - 2 * n) * G, (la + lb) * G)


CALLS = ("fill", "score", "band")


def frame_cols(la: int, call: str) -> int:
    """Columns of the widest frame a call's kernels de-trend over: 1 024, and 4 096 where a call that fills whole matrices
    (`fill`: the fill, nw_batch and sw_batch families) meets a seq_a of 1 024 letters or more (the workgroup fill's frame)."""
    return FILL_FRAME_COLS if call == "fill" and la >= FRAME_COLS else FRAME_COLS


def detrend_cols(spec: dict, la: int, lb: int, call: str) -> int:
    """How many columns of gap_extend the de-trend can add to a cell: with gap_extend <= 0 the trend grows with the position
    inside the frame, which stays below the row's len_a + 1 columns (`band`: below the band's at most len_a + len_b + 1
    diagonals); with gap_extend > 0 it is taken from the frame's far end, whatever the row."""
    cap = frame_cols(la, call)
    return cap if spec["init"][3] > 0 else min(cap, la + lb + 1 if call == "band" else la + 1)


def admitted(spec: dict, la: int, lb: int, call: str = "score") -> bool:
    """The documented rule, restated: value_bound + detrend_cols * |gap_extend| <= INT32_MAX, la and lb the call's longest."""
    return value_bound(spec, la, lb) + detrend_cols(spec, la, lb, call) * abs(spec["init"][3]) <= INT32_MAX


def must_be_admitted(cs, call: str = "score") -> bool:
    """The groups no rule may refuse: the exact peak of every pair plus frame_cols |gap_extend| plus |gap_open| stays below
    2^31 - 1."""
    go, ge = cs[0].spec["init"][2:4]
    la, _ = group_lengths(cs)
    return max(exact(c).peak for c in cs) + frame_cols(la, call) * abs(ge) + abs(go) < INT32_MAX


# ------------------------------------------------------------------------------------------------------------- bands ---
def sw_bands(shape: str, kind: str):
    """[(diag_lo, diag_hi, holds)] for a planted pair: the diagonals the planted path stands on and one more each side; only
    the diagonal it ends on and those above; only the one it starts on."""
    a, b = pair(shape, kind)
    d_end = len(a) - len(b)
    if kind == "both":          # diagonal 0, then 1, then 0 again
        return [(-1, 2, True), (0, 0, False), (1, 6, False)]
    d_start = d_end - 1 if kind == "gapb" else d_end + 1
    lo, hi = min(d_start, d_end), max(d_start, d_end)
    return [(lo - 1, hi + 1, True), (hi, hi + 5, False), (lo, lo, False)]


def nw_bands(shape: str, kind: str):
    """[(w, holds)]: the NW band of width w always spans the diagonals 0 .. len_a - len_b; gapb stays on them, gapa and `both`
    step one diagonal beyond (gapa's seq_a is one letter longer in front of the gap) and are cut at w = 0."""
    return [(0, True), (2, True)] if kind == "gapb" else [(0, False), (1, True), (3, True)]
