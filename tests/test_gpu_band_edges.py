"""GPU tier: banded NW, the exact definition on both band edges at every frame class (band_rows_kernel, sa_band.hip).

test_gpu_band.py checks the wide frames through the in-band property, which a fill that leaks one diagonal past its band, or
cuts one short, still satisfies.  Here every width on both sides of every step of the columns-per-lane ladder runs four
constructed pairs against bandlib's restatement of the definition -- score and both strings:

    upper edge:  a = P + G + Q + S + tail letters,  b = P + Q + G' + S
    lower edge:  a = P + Q + G' + S + tail letters, b = P + G + Q + S

P, S anchors, G, G' unrelated inserts of g letters, Q a shared core: between the inserts the true path runs g diagonals off
the main one.  touch: g is the edge diagonal (d_hi, or -d_lo), so the unbanded alignment lies in the band, on its outermost
diagonal, and a fill that cuts that diagonal loses it.  leak: g is one more, so the band costs the path its core, and a fill
that lets one diagonal more through finds it again.  Each of these is asserted on the reference before the device is asked.

A fifth pair is for the cell left of the frame, which is the floor once the frame has left the border column.  Were it the
border column's value of that row -- the cost of one gap straight down from the origin -- no pair above would notice: behind
their anchor P every band cell is reached for less.  So

    feed:        a = J + Q + G' + S + tail letters,  b = G + Q + S,  |G| = |J| + w, no letter of J scores well against G's

puts the core on the lowest diagonal behind letters that cannot be aligned: inside the band its first cell costs a gap of w
and then |J| mismatches, or two gaps of |J| more; through the cell left of it, one gap of |J| + w and one step.  Asserted on
the reference: bandlib's fill with that defect switched on (border_feed) scores strictly higher.  Where a gap letter costs
more than half a mismatch (gap_extend -3 against mismatch -4) the straight gap never wins and no pair can notice: that
scoring runs the four pairs only.
"""
import random

import pytest

import bandlib as BL
import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W
from test_gpu_band import EDGE_WIDTHS

pytestmark = pytest.mark.gpu

ALPHA = b"ARNDCQEGHILKMFPSTWYV"       # 20 letters: a core off its diagonal scores far below zero, at any band width
SCORINGS = {
    "plain": {"init": [5, -4, -4, -1, 0, 0, 0, 0, 0, 0]},
    "blosum62": {"preset": "BLOSUM62"},
    "free_ends": {"init": [5, -4, -4, -1, 1, 1, 0, 0, 0, 0]},
    "open_pays": {"init": [5, -4, 2, -3, 0, 0, 0, 0, 0, 0]},     # gap_open > 0: the general path
}
OTHER_WIDTHS = [65, 193, 385, 513, 1024]
FEED_JUNK = 40                        # |J|
FEED_A, FEED_B = b"W", b"RNDEKPST"    # J's and G's letters: every pair of them scores -4 (BLOSUM62: -2 .. -4)
MOVING_ROWS = 130                     # rows after the frame starts to move: two refetches of the row and entering-column codes
CPLS = (1, 2, 3, 4, 5, 6, 8, 12, 16)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def build_pair(rng, width, side, kind, q_extra, free_ends=False):
    """(a, b, w, tested edge diagonal as a distance from the main one).  With free start and end gaps an anchor of n letters
    is worth aligning (5 n, for a gap of g: -4 - g) only while that beats stepping over it (-4 - n), so while 6 n > g:
    shorter anchors are skipped, the unbanded path overshoots diagonal g by n, and no touch pair exists."""
    w, tail = (width - 1) // 2, (width - 1) % 2
    edge = w + tail if side == "upper" else w
    g = edge + (kind == "leak")
    rand = lambda n: bytes(rng.choice(ALPHA) for _ in range(n))
    if kind == "feed":
        J = bytes(rng.choice(FEED_A) for _ in range(FEED_JUNK))
        G = bytes(rng.choice(FEED_B) for _ in range(FEED_JUNK + w))
        G2, Q = rand(w), rand(w // 2 + 80 + q_extra)
        S_ = rand(max(10, MOVING_ROWS + w + 1 - (len(G) + len(Q))))
        return J + Q + G2 + S_ + rand(tail), G + Q + S_, w, edge
    anchor = 10 + g // 5 if free_ends else 10
    P, G, G2, Q = rand(anchor), rand(g), rand(g), rand(g // 2 + 80 + q_extra)
    S_ = rand(max(anchor, MOVING_ROWS + w + 1 - (len(P) + g + len(Q))))
    with_g, without = P + G + Q + S_, P + Q + G2 + S_
    a, b = (with_g, without) if side == "upper" else (without, with_g)
    return a + rand(tail), b, w, edge


def check_reference(osc, a, b, w, side, kind, edge):
    """(the reference-only conditions that one pair misses, the banded score, the banded alignment)."""
    la, lb = len(a), len(b)
    d_lo, d_hi = BL.band_of(la, lb, w)
    want_score, want = BL.expected_both(osc, a, b, w)
    fails = []
    if (d_hi if side == "upper" else -d_lo) != edge:
        fails.append(("edge", d_lo, d_hi, edge))
    if lb + d_lo - 1 < MOVING_ROWS:
        fails.append(("moving rows", lb + d_lo - 1))
    if want is None or want[0] != want_score:
        fails.append(("no alignment in the band", want_score))
    if kind == "feed":
        gain = BL.expected_score(osc, a, b, w, border_feed=True) - want_score
        if gain <= 0:
            fails.append(("a border value left of the band gains nothing", gain))
    elif kind == "leak":
        wider = (d_lo, d_hi + 1) if side == "upper" else (d_lo - 1, d_hi)
        gain = BL.expected_score(osc, a, b, w, band=wider) - want_score
        if gain <= 0:
            fails.append(("one diagonal more gains nothing", gain))
    else:
        rc, score, ra, rb = O.oracle_nw(osc, a, b)
        lo, hi = BL.excursion(ra, rb)
        if rc != 0 or not BL.in_band(ra, rb, la, lb, w):
            fails.append(("the unbanded alignment leaves the band", lo, hi, d_lo, d_hi))
        elif (hi if side == "upper" else -lo) != edge:
            fails.append(("the unbanded alignment stays off the edge", lo, hi, edge))
        elif want != (score, ra, rb):
            fails.append(("in band, and not the oracle's", want[0], score))
    return fails, want_score, want


def edge_cases(name, width):
    """The five (open_pays: four) pairs of one width under one scoring, each with its reference results.  A pair that misses a condition is
    built again with a longer core (the conditions are asserted by the caller on what is kept)."""
    sc = S.make_scoring(SCORINGS[name])
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    cases = []
    kinds = [("upper", "touch"), ("upper", "leak"), ("lower", "touch"), ("lower", "leak")] + [("lower", "feed")] * (name != "open_pays")
    for side, kind in kinds:
        for attempt in range(6):
            rng = random.Random(f"{name} {width} {side} {kind} {attempt}")
            a, b, w, edge = build_pair(rng, width, side, kind, 60 * attempt, name == "free_ends")
            fails, want_score, want = check_reference(osc, a, b, w, side, kind, edge)
            if not fails:
                break
        cases.append(dict(side=side, kind=kind, a=a, b=b, w=w, fails=fails, want_score=want_score, want=want, attempt=attempt))
    return sc, cases


def run_width(ctx, name, width):
    sc, cases = edge_cases(name, width)
    for c in cases:
        la, lb = len(c["a"]), len(c["b"])
        assert not c["fails"], (name, width, c["side"], c["kind"], c["fails"])
        assert la - lb == (width - 1) % 2 and BL.width_of(la, lb, c["w"]) == width
        assert BL.band_of(la, lb, c["w"]) == (-c["w"], c["w"] + la - lb)
    batch = W.from_pairs([(c["a"], c["b"]) for c in cases])
    bands = [c["w"] for c in cases]
    tags = [(c["side"], c["kind"]) for c in cases]
    score = [int(s) for s in ctx.nw_score_banded(batch, sc, bands)]
    ran_score = ctx.last_call()
    print(f"{name} width {width}: want {[c['want_score'] for c in cases]} score {score} rebuilt {[c['attempt'] for c in cases]}")
    bad = [(t, s, c["want_score"]) for t, s, c in zip(tags, score, cases) if s != c["want_score"]]
    assert not bad, ("nw_score_banded", name, width, bad)
    got = ctx.nw_align_banded(batch, sc, bands)
    ran_align = ctx.last_call()
    bad = [(t, g[0], c["want"][0]) for t, g, c in zip(tags, got, cases) if g != c["want"]]
    assert not bad, ("nw_align_banded", name, width, bad)
    # what ran: all the pairs are in one width class, so one launch each
    assert len(cases) == (4 if name == "open_pays" else 5)
    assert ran_score == {"band_score": (1, len(cases))}, ran_score
    assert ran_align == {"band_fill": (1, len(cases)), "band_walk": (1, len(cases))}, ran_align


@pytest.mark.parametrize("width", EDGE_WIDTHS)
def test_both_edges_at_every_width(ctx, width):
    """63, 1 023 and both sides of every step of the ladder, match 5 / mismatch -4 / gap_open -4 / gap_extend -1."""
    assert len(EDGE_WIDTHS) == 19
    run_width(ctx, "plain", width)


@pytest.mark.parametrize("width", OTHER_WIDTHS)
@pytest.mark.parametrize("name", ["blosum62", "free_ends", "open_pays"])
def test_both_edges_other_scorings(ctx, name, width):
    """A substitution table, free start and end gaps, and gap_open > 0 (the general sweep) on five of the widths."""
    run_width(ctx, name, width)


def test_one_launch_per_width_class(ctx):
    """The five pairs of several widths in one batch: one band_score / band_fill launch per class of columns per lane."""
    sc, cases = None, []
    for width in (63, 129, 385):
        sc, more = edge_cases("plain", width)
        cases += more
    assert not any(c["fails"] for c in cases)
    classes = {next(c for c in CPLS if 64 * c >= BL.width_of(len(x["a"]), len(x["b"]), x["w"])) for x in cases}
    assert classes == {1, 3, 8}
    batch = W.from_pairs([(c["a"], c["b"]) for c in cases])
    bands = [c["w"] for c in cases]
    score = [int(s) for s in ctx.nw_score_banded(batch, sc, bands)]
    assert ctx.last_call() == {"band_score": (3, 15)}, ctx.last_call()
    got = ctx.nw_align_banded(batch, sc, bands)
    ran = ctx.last_call()
    assert ran["band_fill"] == (3, 15) and ran["band_walk"][1] == 15 and set(ran) == {"band_fill", "band_walk"}, ran
    assert score == [c["want_score"] for c in cases] and got == [c["want"] for c in cases]
