"""Helpers of the banded NW statistics tests (seqalign_nw_stats_banded).  Not a test module.

want                what the call must return for one pair: (score, matches, mismatches) -- the banded end value
                    (bandlib.expected_both) and the counted columns (statlib.count_columns) of the oracle's walk over the banded
                    matrices -- or None where that walk finds no alignment inside the band: the call returns
                    SEQALIGN_E_TRACEBACK.  The rule is the WALK's: it fails, or (no_mismatches only, the documented family) it
                    "succeeds" along the floor -- through a blocked letter pair or out of the band (walked_along_the_floor).
                    The end value does not decide: at large
                    scales a real score lies below INT32_MIN / 2 (tests/maglib.py, the deep families);
below_half          the rule the call followed before -- the end value is below INT32_MIN / 2 -- kept for
                    test_magnitude_argument_cpu.py, which holds the two rules together on every case list of the banded NW
                    statistics tests that runs under a scoring that forbids moves;
frame_model         the kernel's bookkeeping (sa_band_nw_stats.hip) in pure Python over payloads (matches,
                    mismatches, mark), values from bandlib.fill: frame positions, the three phases of the feed, the shift, the
                    reset of V AND D of the cell above the right edge, the end pick at position len_a - fc(len_b).  Modelled on
                    bandstatlib.frame_model and statlib.kernel_model.  A position that holds no band cell carries POISON, so a
                    band cell that read one would show it;
small_pairs         the CPU tier's pairs with a band each: len_a < len_b and len_a > len_b, widths 1 .. max_width;
flag_pairs          the GPU tier's 40 mixed-case pairs per flag combination, at widths 69 / 70;
row_flag_triples    the GPU tier's four pairs at width 385 for one flag that changes the row;
bandless_pair       a sequence and its copy with one substitution: no alignment where mismatches and gaps are forbidden;
counts_reversed_differ, tie_batch, tie_counts   the tie-dense batches of the GPU tier (statlib.tie_pairs) and, per batch and
                    band, how many pairs change their counts under the reversed priority M > B > A over the BANDED matrices
                    (statlib.walk(mats=...)).
"""
from __future__ import annotations

import random

import bandlib as BL
import statlib as ST

HALF = -(1 << 30)            # INT32_MIN / 2
POISON = None
Z, MARK = (0, 0, False), (0, 0, True)
BORDER, STOPPED, MOVING = "border", "stopped", "moving"      # the three phases of the feed


def below_half(osc, a: bytes, b: bytes, w: int) -> bool:
    """The former rule: the banded end value is below INT32_MIN / 2."""
    return BL.expected_both(osc, a, b, w)[0] < HALF


def walked_along_the_floor(osc, a: bytes, b: bytes, w: int, ra: bytes, rb: bytes) -> bool:
    """The documented family (include/seqalign_hip.h, banded NW statistics): under no_mismatches the align walker reads a
    blocked letter pair as score 0, floor + 0 == floor lets it step from a cell at the floor to any other, cells outside the
    band included, and the walk "succeeds".  Such strings are no alignment of the banded problem, and they show it: they hold
    a column of two letters that the scoring does not call a match, or they leave the band (a walk that only follows real
    candidates never does: outside the band every state holds the floor, which no candidate above the floor descends from)."""
    if not BL.in_band(ra, rb, len(a), len(b), w):
        return True
    look = ST.Lookup(osc)
    return bool(osc.no_mismatches) and any(x != 45 and y != 45 and not look(x, y)[1] for x, y in zip(ra, rb))


def want_walked(osc, a: bytes, b: bytes, w: int):
    """((score, matches, mismatches), (score, gapped a, gapped b) of the oracle's walk), or None: the oracle's walk over the
    banded matrices fails, or runs along the floor (walked_along_the_floor)."""
    value, walked = BL.expected_both(osc, a, b, w)
    if walked is None or walked_along_the_floor(osc, a, b, w, walked[1], walked[2]):
        return None
    assert walked[0] == value, (a, b, w, value, walked)
    return (value,) + ST.count_columns(osc, walked[1], walked[2]), walked


def want(osc, a: bytes, b: bytes, w: int):
    """(score, matches, mismatches), or None: no alignment inside the band."""
    both = want_walked(osc, a, b, w)
    return None if both is None else both[0]


def frame_model(osc, a: bytes, b: bytes, w: int, F: int = 8):
    """((score, matches, mismatches), whether the end state carries the mark, the phases of the feed the rows went through) the
    way band_nw_stats_rows_kernel finds them with a frame of F positions."""
    la, lb = len(a), len(b)
    W_ = la + 1
    d_lo, d_hi = BL.band_of(la, lb, w)
    assert d_hi - d_lo + 1 <= F
    M, A, B = (X.tolist() for X in BL.fill(osc, a, b, (d_lo, d_hi)))
    score = ST.end_pick(M, A, B, W_ * (lb + 1) - 1)[1]
    if la == 0:                                              # the border column is the whole matrix
        return (score, 0, 0), False, set()
    fl = ST.floor_of(osc)
    open1, ext = osc.gap_open + osc.gap_extend, osc.gap_extend
    no_end, nga, ngb, no_mm = bool(osc.no_end_gap_penalty), bool(osc.no_gaps_in_a), bool(osc.no_gaps_in_b), bool(osc.no_mismatches)
    look = ST.Lookup(osc)
    fa, fb = ST.fold(osc, a), ST.fold(osc, b)

    def merge(l, r):                                         # l lies left of r: r wins a tie only as an opening from A
        return l if l[0] >= r[0] + r[1] else r

    # row 0: the frame stands at column 1; columns 1 .. d_hi are band cells of the border
    D = [Z if 1 + g <= min(la, d_hi) else POISON for g in range(F)]
    V = list(D)
    bound_d = Z                                              # cell (0, 0)
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
            feed = dict(z=max(M[r], A[r]), b=B[r], from_a=True, zs=Z, bs=Z)
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
        run, zl = None, feed
        for g in range(n_row):
            x = fc + g
            m, av, bv = M[r + x], A[r + x], B[r + x]
            a_ok = (not nga) or x == la
            pd, pu = r - W_ + x - 1, r - W_ + x
            s, is_match = look(a[x - 1], b[j - 1])
            eq = fa[x - 1] == fb[j - 1]
            assert dprev is not POISON, ("D of the up-left", x, j)
            if (no_mm and not is_match) or max(M[pd], A[pd], B[pd]) + s < fl:
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
                    cand = (fl, 0, MARK)                     # clamped: the floor loses a tie to every candidate
                if g == 0:
                    cand = merge((feed["b"] + step, 1, feed["bs"]), cand)
                if run is not None:
                    cand = merge((run[0] + step, run[1], run[2]), cand)
                run = cand
                assert run[0] == bv, (x, j, run, bv)
                bs = run[2]
            assert POISON not in (ms, as_, bs), (x, j)       # a band cell never reads a position without one
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
    m, mm, mark = D[at]
    return (score, m, mm), mark, phases


# ------------------------------------------------------------------------------------------------------- CPU tier pairs ---
def _rand_seq(rng, n, alpha):
    return bytes(rng.choice(alpha) for _ in range(n))


def _mutate(rng, s, alpha):
    out = bytearray()
    for ch in s:
        r = rng.randrange(14)
        if r == 0:
            continue
        if r == 1:
            out += _rand_seq(rng, 1 + rng.randrange(2), alpha)
        out.append(rng.choice(alpha) if r == 2 else ch)
    return bytes(out)


def small_pairs(seed: int, n: int, alpha: bytes, max_len: int = 20, max_width: int = 8):
    """[(a, b, w)]: random pairs and relatives with |len_a - len_b| < max_width and every w whose band is at most max_width
    diagonals wide drawn with equal chance; the degenerate pairs at the end."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        la = rng.randrange(max_len + 1)
        a = _rand_seq(rng, la, alpha)
        b = _mutate(rng, a, alpha)[:max_len] if len(out) % 2 else _rand_seq(rng, rng.randrange(max_len + 1), alpha)
        ws = [w for w in range(max_width) if BL.width_of(len(a), len(b), w) <= max_width]
        if ws:
            out.append((a, b, rng.choice(ws)))
    one = alpha[:1]
    return out + [(b"", b"", 0), (one, b"", 0), (b"", one, 0), (one, one, 0), (one * 3, b"", 2), (b"", one * 3, 1)]


# ------------------------------------------------------------------------------------------------------- GPU tier inputs ---
FLAG_N = 40


def flag_pairs(idx: int, flags, alpha: bytes):
    """[(a, b, w)], FLAG_N mixed-case pairs of 80 .. 120 letters at widths 69 / 70 for the idx-th flag combination (no_start,
    no_end, no_gaps_in_a, no_gaps_in_b, no_mismatches).  Most pairs are relatives with 10 % edits.  Where the scoring forbids
    mismatches AND a kind of gap such a pair rarely keeps an alignment, so there four of five pairs differ only by what hangs
    over at the two ends and by case; test_nw_stats_banded_argument_cpu.py asserts on the oracle how many pairs each batch
    loses."""
    rng = random.Random(7100 + idx)
    strict = flags[4] and (flags[2] or flags[3])
    case_sensitive = idx & 1                                 # bandspanlib.flag_scoring
    out = []
    for k in range(FLAG_N):
        la = rng.randrange(80, 111)
        a = _rand_seq(rng, la, alpha)
        edited = (k % 5 == 0) if strict else (k % 5 != 4)
        if edited:
            b = BL.mutate(rng, a, 0.10, alpha)
        else:
            # at either end ONE of the two hangs over: with both kinds of gap forbidden a gap may stand in row 0 or column 0,
            # in the last row or the last column, and nowhere else
            head, tail = rng.randrange(-5, 6), rng.randrange(-5, 6)
            core = a[max(head, 0):la - max(tail, 0)]
            if not case_sensitive:
                core = bytes(ch ^ 0x20 if rng.random() < 0.3 else ch for ch in core)     # the other case
            b = _rand_seq(rng, max(-head, 0), alpha) + core + _rand_seq(rng, max(-tail, 0), alpha)
        b = b[:120]
        w = (69 - abs(len(a) - len(b))) // 2
        assert BL.width_of(len(a), len(b), w) in (69, 70), (len(a), len(b), w)
        out.append((a, b, w))
    return out


ROW_FLAGS = ("no_gaps_in_a", "no_gaps_in_b", "no_mismatches", "no_end")


def row_flag_triples(flag: str):
    """[(a, b, w)], four pairs of 275 .. 300 rows at width 385 (w = 192 on equal lengths, 191 two apart) for one of ROW_FLAGS.
    len_a > d_hi, so the band's right edge meets the last column."""
    rng = random.Random(385 + len(flag))
    out = []
    for d in (0, 2, -2, 0):                                  # len_b - len_a: even, so that 385 = |d| + 1 + 2 w
        a = _rand_seq(rng, rng.randrange(275, 300), b"ACGT")
        b = (BL.mutate(rng, a, 0.08) + _rand_seq(rng, len(a), b"ACGT"))[:len(a) + d]
        out.append((a, b, 192 - abs(d) // 2))
    assert all(BL.width_of(len(a), len(b), w) == 385 and len(a) > BL.band_of(len(a), len(b), w)[1] for a, b, w in out)
    return out


def bandless_pair(n: int, at: int):
    """(s, t): n random letters and the same with the letter at `at` replaced -- under a scoring that forbids mismatches and both
    kinds of gap the pair has no alignment inside any band."""
    s = _rand_seq(random.Random(4), n, b"ACGT")
    return s, s[:at] + bytes([b"ACGT"[(b"ACGT".index(s[at]) + 1) % 4]]) + s[at + 1:]


def counts_reversed_differ(osc, a: bytes, b: bytes, w: int) -> bool:
    """Whether the pair's banded (matches, mismatches) change when the predecessor priority is reversed to M > B > A."""
    mats = BL.fill(osc, a, b, BL.band_of(len(a), len(b), w))
    return ST.walk(osc, a, b, ST.WALKER, mats) != ST.walk(osc, a, b, ST.REVERSED, mats)


TIE_WIDTHS = (64, 200)
TIE_BANDS = (3, 20, 150)     # the widest: |len_a - len_b| <= 103 at width 200, so at most 404 diagonals
# (scoring, width) -> pairs taken from statlib.tie_pairs' generator where its first 40 hold none that is tie-sensitive inside
# every band; a batch is lengthened, never thinned
TIE_N: dict = {}


def tie_batch(name: str, width: int):
    return ST.tie_pairs(name, width, n=TIE_N.get((name, width), 40))


def tie_counts(osc_of):
    """{(scoring name, width, w): pairs of tie_batch(name, width) whose counts are tie-sensitive inside the band}."""
    out = {}
    for name in ST.TIE_SCORINGS:
        osc = osc_of(name)
        for width in TIE_WIDTHS:
            pairs = tie_batch(name, width)
            for w in TIE_BANDS:
                out[name, width, w] = sum(counts_reversed_differ(osc, a, b, w) for a, b in pairs)
    return out
