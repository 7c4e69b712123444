"""GPU tier: the banded calls, narrow (sa_band.hip) and wide (sa_band_strips.hip), and seqalign_sw_align_long
(sa_align_long.hip) on gap-dense pairs.

None of these calls met a pair whose alignment puts an insertion run directly against a deletion run, except
nw_align_banded and nw_align_long once each (tests/test_gpu_gap_dense.py).  A band does something new to such a pair: under
(0, +1) the alternation's hit keeps its I->D transitions, under (-1, 0) the same score is reached through D->I only -- a move
order alignment_reverse_move never produces without a band -- and under (0, 0) the hit collapses to a few columns
(tests/test_span_band_dense_argument_cpu.py).  With strips of 64 columns the spaced pairs put those transitions in every
column of a strip.  Every case compares with the definitions (bandswlib.expected, bandlib.expected, orclib.oracle_sw /
oracle_nw), the wide calls with the narrow ones byte for byte, and asserts what seqalign_ctx_last_call_info says ran.
"""
import pytest

import bandlib as BL
import bandswlib as BS
import denselib as D
import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W
from test_gpu_band_wide import run

pytestmark = pytest.mark.gpu

STRIP = 64
NW_BANDS = (0, 1, 3, 40)
NW_OF = {"swdense": "cheap0", "ties": "ties", "ext0": "ext0"}      # the NW scoring run on a SW scoring's pairs (same matches_of)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


_SC, _SW, _NW = {}, {}, {}


def scoring(name):
    if name not in _SC:
        _SC[name] = S.make_scoring(D.SCORINGS[name])
    return _SC[name]


def want_sw(name, a, b, lo, hi):
    """bandswlib.expected, once per (scoring, pair, band) for the whole file: ((score, end_a, end_b), hit or None)."""
    key = (name, a, b, lo, hi)
    if key not in _SW:
        _SW[key] = BS.expected(D.oracle_scoring(name), a, b, lo, hi)
    return _SW[key]


def want_nw(name, a, b, w):
    key = (name, a, b, w)
    if key not in _NW:
        _NW[key] = BL.expected(D.oracle_scoring(name), a, b, w)
    return _NW[key]


def pairs_of(la, lb, name):
    return D.band_pairs(la, lb, name) + D.band_added(la, lb, name)


def cells_of(res, n):
    return [(int(res[0][p]), int(res[1][p]), int(res[2][p])) for p in range(n)]


def strips_sw(pairs, lo, hi):
    """Busy strips of 64 columns of the wide SW calls: the columns max(1, 1 + d_lo) .. min(len_a, len_b + d_hi) of each pair."""
    total = 0
    for a, b in pairs:
        band = BS.clip(len(a), len(b), lo, hi)
        cols = 0 if band is None or not b else max(0, min(len(a), len(b) + band[1]) - max(1, 1 + band[0]) + 1)
        total += -(-cols // STRIP)
    return total


def ran_wide(info, kinds, low, n):
    """The wide kernels count strips, the narrow ones pairs: `low` busy strips (more than n pairs) in one launch."""
    first = kinds[0]
    return set(info) == set(kinds) and info[first][0] == 1 and n < low <= info[first][1] <= low + n and (len(kinds) == 1 or info["band_walk"] == (1, n))


SHAPES = pytest.mark.parametrize("shape", D.BAND_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
NAMES = pytest.mark.parametrize("name", D.SW_SCORINGS)


# ---------------------------------------------------------------- B1. banded SW, narrow --
@SHAPES
@NAMES
def test_banded_sw_on_gap_dense_pairs(ctx, name, shape):
    """sw_score_banded and sw_align_banded on six alternation and two spaced pairs under seven bands: the whole matrix (which
    is sw_batch's first hit), the hit's excursion and one diagonal more, exactly it (I->D), its mirror (D->I), the main
    diagonal alone, a wide band, a band beside the main diagonal."""
    la, lb = shape
    pairs = pairs_of(la, lb, name)
    n = len(pairs)
    batch = W.from_pairs(pairs)
    for lo, hi in D.sw_bands(la, lb):
        want = [want_sw(name, a, b, lo, hi) for a, b in pairs]
        cells = cells_of(ctx.sw_score_banded(batch, scoring(name), lo, hi), n)
        assert ctx.last_call() == {"band_score": (1, n)}, (lo, hi, ctx.last_call())
        assert cells == [w[0] for w in want], (name, shape, lo, hi)
        hits = ctx.sw_align_banded(batch, scoring(name), lo, hi, 1)
        assert ctx.last_call() == {"band_fill": (1, n), "band_walk": (1, n)}, (lo, hi, ctx.last_call())
        bad = [(p, hits[p], want[p][1]) for p in range(n) if hits[p] != ([want[p][1]] if want[p][1] else [])]
        assert not bad, (name, shape, lo, hi, bad[:2])
        if (lo, hi) == (-lb, la):
            assert hits == ctx.sw_batch(batch, scoring(name), 1, max_hits=1)
            assert "band_fill" not in ctx.last_call()
            for (a, b), h in zip(pairs, hits):
                assert (0, h) == O.oracle_sw(D.oracle_scoring(name), a, b, 1, 1)


# ---------------------------------------------------------------- B2. the wide calls, strips of 64 columns --
@SHAPES
@NAMES
def test_wide_banded_sw_on_gap_dense_pairs(ctx, name, shape):
    """The two wide SW calls on B1's pairs and bands with band_strip_cols = 64: the definitions' results, and the narrow
    calls' byte for byte."""
    la, lb = shape
    pairs = pairs_of(la, lb, name)
    n = len(pairs)
    batch = W.from_pairs(pairs)
    for lo, hi in D.sw_bands(la, lb):
        want = [want_sw(name, a, b, lo, hi) for a, b in pairs]
        low = strips_sw(pairs, lo, hi)
        with ctx.options(band_strip_cols=STRIP):
            score = run(ctx.sw_score_banded_wide, batch, scoring(name), lo, hi)
            assert ran_wide(ctx.last_call(), ("band_score",), low, n), (lo, hi, low, ctx.last_call())
            hits = run(ctx.sw_align_banded_wide, batch, scoring(name), lo, hi, 1)
            assert ran_wide(ctx.last_call(), ("band_fill", "band_walk"), low, n), (lo, hi, low, ctx.last_call())
        assert cells_of(score, n) == [w[0] for w in want], (name, shape, lo, hi)
        assert hits == [[w[1]] if w[1] else [] for w in want], (name, shape, lo, hi)
        narrow = ctx.sw_score_banded(batch, scoring(name), lo, hi)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(score, narrow))
        assert hits == ctx.sw_align_banded(batch, scoring(name), lo, hi, 1)


@SHAPES
@NAMES
def test_wide_banded_nw_on_gap_dense_pairs(ctx, name, shape):
    """The two wide NW calls on the same pairs under bands 0, 1, 3 and 40 with band_strip_cols = 64: bandlib's results, the
    narrow calls' byte for byte, and from band 3 on nw_batch's."""
    la, lb = shape
    nw = NW_OF[name]
    assert D.matches_of(nw) == D.matches_of(name)
    pairs = pairs_of(la, lb, name)
    n = len(pairs)
    batch = W.from_pairs(pairs)
    low = n * -(-la // STRIP)
    full = ctx.nw_batch(batch, scoring(nw))
    for (a, b), got in zip(pairs, full):
        assert (0, *got) == O.oracle_nw(D.oracle_scoring(nw), a, b)
    for w in NW_BANDS:
        want = [want_nw(nw, a, b, w) for a, b in pairs]
        assert all(x is not None for x in want)
        with ctx.options(band_strip_cols=STRIP):
            score = run(ctx.nw_score_banded_wide, batch, scoring(nw), w)
            assert ran_wide(ctx.last_call(), ("band_score",), low, n), (w, low, ctx.last_call())
            got = run(ctx.nw_align_banded_wide, batch, scoring(nw), w)
            assert ran_wide(ctx.last_call(), ("band_fill", "band_walk"), low, n), (w, low, ctx.last_call())
        assert got == want, (name, shape, w)
        assert [int(s) for s in score] == [x[0] for x in want]
        assert score.tobytes() == ctx.nw_score_banded(batch, scoring(nw), w).tobytes()
        assert ctx.last_call() == {"band_score": (1, n)}, ctx.last_call()
        assert got == ctx.nw_align_banded(batch, scoring(nw), w)
        assert ctx.last_call() == {"band_fill": (1, n), "band_walk": (1, n)}, ctx.last_call()
        if w >= 3:          # the bands that hold the unbanded alignment (test_span_band_dense_argument_cpu.py)
            assert got == full, (name, shape, w)


def test_wide_nw_band_3_holds_the_alternation(ctx):
    """test_nw_align_banded_holds_the_alternation's pairs through the wide call at strips of 64 columns: nw_batch's result byte
    for byte."""
    pairs = [D.alternation(150, 150, k) for k in range(12)] + [D.alternation(500, 500, 2), D.spaced(150, 150, 12, 3)]
    batch = W.from_pairs(pairs)
    with ctx.options(band_strip_cols=STRIP):
        got = run(ctx.nw_align_banded_wide, batch, scoring("cheap0"), 3)
        info = ctx.last_call()
    low = sum(-(-len(a) // STRIP) for a, b in pairs)
    assert ran_wide(info, ("band_fill", "band_walk"), low, len(pairs)), (low, info)
    assert got == ctx.nw_batch(batch, scoring("cheap0"))
    for (a, b), g in zip(pairs, got):
        assert (0, *g) == O.oracle_nw(D.oracle_scoring("cheap0"), a, b) and D.count_id(g[1], g[2]) >= 8


@pytest.mark.parametrize("cols", [64, 0])
def test_dense_pair_past_the_narrow_cap(ctx, cols):
    """alternation(1 300, 1 300) at 1 201 diagonals: SW under [5,-10,0,-1] within (-600, 600), NW under [2,-9,0,-1] with band
    600 (648 I->D), strips of 64 columns and the default.  The narrow calls refuse the pair; no wide call may time out."""
    la, lb = D.PAST_CAP["shape"]
    a, b = D.alternation(la, lb)
    batch = W.from_pairs([(a, b)])
    sw, lo, hi = D.PAST_CAP["sw"]
    nw, w = D.PAST_CAP["nw"]
    for refused in (lambda: ctx.sw_score_banded(batch, scoring(sw), lo, hi), lambda: ctx.nw_score_banded(batch, scoring(nw), w)):
        with pytest.raises(S.SeqAlignError) as e:
            refused()
        assert e.value.code == S.E_TOO_LARGE
    cell, hit = want_sw(sw, a, b, lo, hi)
    alignment = want_nw(nw, a, b, w)
    with ctx.options(band_strip_cols=cols):
        score = run(ctx.sw_score_banded_wide, batch, scoring(sw), lo, hi)
        assert set(ctx.last_call()) == {"band_score"} and ctx.last_call()["band_score"][0] == 1, ctx.last_call()
        assert cells_of(score, 1) == [cell]
        assert run(ctx.sw_align_banded_wide, batch, scoring(sw), lo, hi, 1) == [[hit]]
        assert set(ctx.last_call()) == {"band_fill", "band_walk"} and ctx.last_call()["band_walk"] == (1, 1), ctx.last_call()
        assert [int(s) for s in run(ctx.nw_score_banded_wide, batch, scoring(nw), w)] == [alignment[0]]
        assert set(ctx.last_call()) == {"band_score"}, ctx.last_call()
        assert run(ctx.nw_align_banded_wide, batch, scoring(nw), w) == [alignment]
        info = ctx.last_call()
        assert set(info) == {"band_fill", "band_walk"} and info["band_walk"] == (1, 1), info
        if cols:
            assert info["band_fill"][1] in (-(-la // cols), -(-la // cols) + 1), info      # 21 strips of 64 columns
    assert D.count_id(hit["a"], hit["b"]) >= 600 and D.count_id(alignment[1], alignment[2]) >= 600


# ---------------------------------------------------------------- B3. sw_align_long --
@pytest.mark.parametrize("rows", [7, 64])
@pytest.mark.parametrize("name", ["swdense", "ties"])
def test_sw_align_long_seams_inside_alternating_stretches(ctx, name, rows):
    """seqalign_sw_align_long with blocks of 7 and 64 rows on test_nw_align_long_seams_inside_alternating_stretches's pairs
    and alternation(1 100, 300): with a period of two rows per 1I1D every block seam falls inside an alternating stretch (7 is
    odd: on either row of the period in turn).  The oracle's first hit at min_score 4, strings and all."""
    pairs = D.long_sw_pairs()
    with ctx.options(long_block_rows=rows):
        got = ctx.sw_align_long(W.from_pairs(pairs), scoring(name), D.SW_MIN_SCORE)
        ran = ctx.last_call()
    assert set(ran) == {"long_forward", "long_block", "long_walk"}, ran
    assert ran["long_block"][0] >= 2, ran
    for p, (a, b) in enumerate(pairs):
        rc, hits = O.oracle_sw(D.oracle_scoring(name), a, b, D.SW_MIN_SCORE, 1)
        assert rc == 0 and got[p] == hits, (name, rows, p, len(a), len(b))
