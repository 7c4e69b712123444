"""GPU tier: banded NW gap-run counts -- seqalign_nw_gaps_banded and seqalign_nw_gaps_banded_wide (sa_band_nw_gaps.hip over
sa_band_nw_frame.hpp, sa_batch_band.hip).

Every result is checked against the oracle -- the banded end value and the '-' runs of its walk over the banded matrices
(nwgaplib.band_want), or SEQALIGN_E_TRACEBACK naming the lowest pair that has no alignment inside its band -- the score
against ctx.nw_score_banded[_wide] byte for byte, the wide call against the narrow one byte for byte wherever the narrow call
accepts the batch, and all three values against ctx.nw_gaps for every pair whose band is the whole matrix.  The shapes are
test_gpu_nw_stats_banded.py's and test_gpu_nw_stats_banded_wide.py's: the smallest at which the frame can go wrong."""
import itertools
import random

import numpy as np
import pytest

import bandlib as BL
import bandnwstatlib as BN
import bandspanlib as BSP
import denselib as D
import nwgaplib as NG
import orclib as O
import seqalign_amd as S
import statlib as ST
import swgaplib as SG
from seqalign_amd import workloads as W
from test_gpu_nw_stats_banded import WIDTHS, width_triples
from test_gpu_nw_stats_banded_wide import geometry_cases

pytestmark = pytest.mark.gpu

PLAIN = [1, -2, -4, -1]
FULL = 2 ** 32 - 1
NARROW_MAX = 512


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def scoring(init4, **flags):
    sc = S.make_scoring(ST.init_spec(init4, **flags))
    return sc, O.Scoring.from_buffer_copy(bytes(sc))


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def run(fn, *args):
    """fn(*args); an error passes through, but never the wide calls' hand-off time-out."""
    try:
        return fn(*args)
    except S.SeqAlignError as e:
        assert "timed out" not in str(e), str(e)
        raise


def same_bytes(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def check(ctx, sc, osc, triples, want=None, wide=False):
    """The call on [(a, b, w)] the ways of the module's header; returns the wanted list (None: no alignment inside the band).
    A batch with such pairs must raise E_TRACEBACK naming the lowest, and is checked without them."""
    call, score_call = (ctx.nw_gaps_banded_wide, ctx.nw_score_banded_wide) if wide else (ctx.nw_gaps_banded, ctx.nw_score_banded)
    want = want or [NG.band_want(osc, a, b, w) for a, b, w in triples]
    none = [p for p, x in enumerate(want) if x is None]
    if none:
        with pytest.raises(S.SeqAlignError) as e:
            run(call, W.from_pairs([(a, b) for a, b, _ in triples]), sc, [w for _, _, w in triples])
        assert e.value.code == S.E_TRACEBACK and f"pair {none[0]}:" in str(e.value), (str(e.value), none)
    kept = [p for p, x in enumerate(want) if x is not None]
    if not kept:
        return want
    batch = W.from_pairs([triples[p][:2] for p in kept])
    bands = [triples[p][2] for p in kept]
    res = run(call, batch, sc, bands)
    assert [r.dtype for r in res] == [np.int32, np.uint32, np.uint32] and all(r.shape == (len(kept),) for r in res)
    got = NG.got_gaps(res)
    bad = [(p, len(triples[p][0]), len(triples[p][1]), triples[p][2], got[k], want[p]) for k, p in enumerate(kept) if got[k] != want[p]]
    assert not bad, (len(bad), bad[:3])
    assert res[0].tobytes() == run(score_call, batch, sc, bands).tobytes()
    widths = [BL.width_of(len(triples[p][0]), len(triples[p][1]), triples[p][2]) for p in kept]
    if wide and max(widths) <= NARROW_MAX:
        assert same_bytes(res, ctx.nw_gaps_banded(batch, sc, bands))
    whole = [k for k, p in enumerate(kept) if widths[k] == len(triples[p][0]) + len(triples[p][1]) + 1]
    if whole:
        full = NG.got_gaps(ctx.nw_gaps(W.from_pairs([triples[kept[k]][:2] for k in whole]), sc))
        assert full == [got[k] for k in whole]
    return want


# ---------------------------------------------------------------- 1. the narrow ladder --
WIDTH_SCORINGS = {"ext0": ([3, -1, -1, 0], b"ARNDCQEGHILKMFPSTWYV"), "dna": (PLAIN, b"ACGT")}


@pytest.mark.parametrize("name", list(WIDTH_SCORINGS))
@pytest.mark.parametrize("width", WIDTHS)
def test_every_width_class_and_its_edges(ctx, width, name):
    """test_gpu_nw_stats_banded.width_triples: both sides of every step of the columns per lane; the alignment along the band's
    left edge, its right edge and its middle; the frame moves across a 64-row code fetch."""
    init, alpha = WIDTH_SCORINGS[name]
    sc, osc = scoring(init)
    want = check(ctx, sc, osc, width_triples(random.Random(1000 + width), width, alpha))
    assert None not in want
    if width > 2:
        assert want[0][1] + want[0][2] > 0 and want[1][1] + want[1][2] > 0, want     # the overhangs are runs


def test_bands_that_hold_and_bands_that_cut_the_alignment(ctx):
    """Relatives with 25 % edits: at the band their unbanded alignment needs the three values are nw_gaps'; at half of it the
    banded result differs on some pair, and is the oracle's."""
    sc, osc = scoring(PLAIN)
    rng = random.Random(5)
    pairs = [(a, BL.mutate(rng, a, 0.25)[:150]) for a in (rand_seq(rng, n) for n in [60, 90, 120, 140, 140, 100, 80, 130])]
    need = []
    for a, b in pairs:
        rc, s, ra, rb = O.oracle_nw(osc, a, b)
        need.append(BL.smallest_band(ra, rb, len(a), len(b)))
    unbanded = NG.want_gaps(osc, pairs)
    holds = check(ctx, sc, osc, [(a, b, w) for (a, b), w in zip(pairs, need)])
    assert holds == unbanded
    assert NG.got_gaps(ctx.nw_gaps(W.from_pairs(pairs), sc)) == unbanded
    cut = check(ctx, sc, osc, [(a, b, w // 2) for (a, b), w in zip(pairs, need)])
    differ = [p for p in range(len(pairs)) if cut[p] != unbanded[p]]
    assert differ and all(cut[p][0] < unbanded[p][0] for p in differ), (cut, unbanded)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("no_start", [0, 1])
def test_empty_sequences_and_a_band_of_one_diagonal(ctx, no_start, wide):
    sc, osc = scoring(PLAIN, no_start=no_start)
    a, b = b"ACGTTGCAAGCTTGCA" * 3, b"GGACGTTGCAAGCTTGCATT" * 2
    triples = [(b"", b, 0), (a, b"", 0), (b"", b"", 0), (b"", b, 9), (a, b"", FULL), (b"", b"", 5),
               (a, a, 0), (a, a[:21] + b"T" + a[22:], 0), (a, b, 0), (b, a, 0), (b"A", b"A", 0), (b"A", b"C", 0), (b"A", b"CC", 0)]
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, triples, wide=wide)
    assert [w[1:] for w in want[:8]] == [(1, 0), (0, 1), (0, 0), (1, 0), (0, 1), (0, 0), (0, 0), (0, 0)], want
    assert want[8][2] >= 1 and want[9][1] >= 1 and want[12][1:] == (1, 0), want     # the longer sequence faces a gap


# ---------------------------------------------------------------- 2. flags --
@pytest.mark.parametrize("idx", range(32))
def test_all_flag_combinations_at_width_70(ctx, idx):
    """bandnwstatlib.flag_pairs: 40 mixed-case pairs; check() asserts the error and the lowest pair, then the batch without
    them, narrow and wide (strips of 64 columns: two per pair)."""
    flags = list(itertools.product([0, 1], repeat=5))[idx]
    spec = BSP.flag_scoring(idx, flags)
    sc = S.make_scoring(spec)
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    triples = BN.flag_pairs(idx, flags, b"ACGTacgt" + (b"N" if spec["wildcards"] else b""))
    want = check(ctx, sc, osc, triples)
    with ctx.options(band_strip_cols=64):
        check(ctx, sc, osc, triples, want, wide=True)
    lost = sum(x is None for x in want)
    assert lost <= BN.FLAG_N // 4 and (lost == 0 or flags[2] or flags[3] or flags[4]), (flags, lost)


@pytest.mark.parametrize("flag", BN.ROW_FLAGS)
def test_flags_that_change_the_row_at_eight_columns_per_lane(ctx, flag):
    sc, osc = scoring(PLAIN, **{flag: 1})
    want = check(ctx, sc, osc, BN.row_flag_triples(flag))
    assert sum(x is not None for x in want) >= 3, want


def test_no_alignment_inside_the_band_names_the_pair(ctx):
    """bandnwstatlib.bandless_pair under no_mismatches and both no_gaps flags: SEQALIGN_E_TRACEBACK with the pair named, as
    nw_stats_banded[_wide] reports it; the context works afterwards."""
    sc, osc = scoring([1, -6, -4, -1], no_mismatches=1, no_gaps_in_a=1, no_gaps_in_b=1)
    s, t = BN.bandless_pair(150, 70)
    triples = [(s, s, 4), (s, s, 0), (s, t, 4), (s, s, 9)]
    for wide in (False, True):
        want = check(ctx, sc, osc, triples, wide=wide)
        assert [x is None for x in want] == [False, False, True, False]
        batch, bands = W.from_pairs([x[:2] for x in triples]), [x[2] for x in triples]
        with pytest.raises(S.SeqAlignError) as ref:
            (ctx.nw_stats_banded_wide if wide else ctx.nw_stats_banded)(batch, sc, bands)
        with pytest.raises(S.SeqAlignError) as err:
            (ctx.nw_gaps_banded_wide if wide else ctx.nw_gaps_banded)(batch, sc, bands)
        assert err.value.code == ref.value.code == S.E_TRACEBACK and "pair 2:" in str(err.value)
        assert str(err.value).split(":", 1)[1] == str(ref.value).split(":", 1)[1]


# ---------------------------------------------------------------- 3. ties --
@pytest.mark.parametrize("w", BN.TIE_BANDS)
@pytest.mark.parametrize("width", BN.TIE_WIDTHS)
@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_inside_a_band(ctx, name, width, w):
    sc, osc = scoring(ST.TIE_SCORINGS[name])
    want = check(ctx, sc, osc, [(a, b, w) for a, b in BN.tie_batch(name, width)])
    assert None not in want


# ---------------------------------------------------------------- 4. wide: strip geometry --
@pytest.fixture(scope="module")
def geometry(ctx):
    """test_gpu_nw_stats_banded_wide.geometry_cases, the oracle's results and the narrow call's (computed once)."""
    pairs, bands = geometry_cases()
    sc, osc = scoring(PLAIN)
    want = [NG.band_want(osc, a, b, w) for (a, b), w in zip(pairs, bands)]
    assert None not in want
    batch = W.from_pairs(pairs)
    narrow = ctx.nw_gaps_banded(batch, sc, bands)
    assert NG.got_gaps(narrow) == want
    return dict(bands=bands, sc=sc, want=want, batch=batch, narrow=narrow)


@pytest.mark.parametrize("cols", [64, 128, 256, 512, 0])
def test_strip_geometry(ctx, geometry, cols):
    g = geometry
    with ctx.options(band_strip_cols=cols):
        res = run(ctx.nw_gaps_banded_wide, g["batch"], g["sc"], g["bands"])
    got = NG.got_gaps(res)
    bad = [(p, int(g["batch"].len_a[p]), int(g["batch"].len_b[p]), g["bands"][p], got[p], g["want"][p])
           for p in range(len(got)) if got[p] != g["want"][p]]
    assert not bad, (len(bad), bad[:5])
    assert same_bytes(res, g["narrow"])


# ---------------------------------------------------------------- 5. wide: past the narrow cap --
@pytest.fixture(scope="module")
def past_caps():
    """Widths 513 to 1 401: 1 300-letter relatives with 6 % edits, an overhang on either side in two of them."""
    rng = random.Random(513)
    sc, osc = scoring(PLAIN)
    cases = []
    for w, tail in ((256, 0), (300, -40), (600, 35), (700, 0)):
        a = rand_seq(rng, 1300)
        b = BL.mutate(rng, a, 0.06)
        cases.append((a + rand_seq(rng, tail), b, w) if tail > 0 else (a, b + rand_seq(rng, -tail), w))
    widths = [BL.width_of(len(a), len(b), w) for a, b, w in cases]
    assert min(widths) > NARROW_MAX and 513 <= min(widths) <= 600 and 1300 <= max(widths) <= 1500, widths
    want = [NG.band_want(osc, a, b, w) for a, b, w in cases]
    a = rand_seq(rng, 700)
    whole = (a, (BL.mutate(rng, a, 0.1) + rand_seq(rng, 100))[:650])
    return sc, osc, cases, want, whole


@pytest.mark.parametrize("cols", [64, 128, 256, 512, 0])
def test_past_the_narrow_cap(ctx, past_caps, cols):
    sc, osc, cases, want, whole = past_caps
    batch, bands = W.from_pairs([c[:2] for c in cases]), [c[2] for c in cases]
    with pytest.raises(S.SeqAlignError) as ref:
        ctx.nw_stats_banded(batch, sc, bands)                  # the narrow calls refuse these, with one message
    with pytest.raises(S.SeqAlignError) as e:
        ctx.nw_gaps_banded(batch, sc, bands)
    assert e.value.code == ref.value.code == S.E_TOO_LARGE and str(e.value).split(":", 1)[1] == str(ref.value).split(":", 1)[1]
    with ctx.options(band_strip_cols=cols):
        check(ctx, sc, osc, cases, want, wide=True)
        aligned = run(ctx.nw_align_banded_wide, batch, sc, bands)
        full = run(ctx.nw_gaps_banded_wide, W.from_pairs([whole]), sc, FULL)
    assert want == [(score,) + SG.gap_runs(ra, rb) for score, ra, rb in aligned]
    assert all(g[1] > 5 and g[2] > 5 for g in want), want
    assert same_bytes(full, ctx.nw_gaps(W.from_pairs([whole]), sc))


# ---------------------------------------------------------------- 6. wide: ties and gaps across seams --
TIE_CASES = ((64, 20), (200, 150), (700, 400))      # (statlib.tie_pairs' width, w): 1, 4 and 11 strips of 64 columns


@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_across_seams(ctx, name):
    sc, osc = scoring(ST.TIE_SCORINGS[name])
    with ctx.options(band_strip_cols=64):
        for width, w in TIE_CASES:
            want = check(ctx, sc, osc, [(a, b, w) for a, b in BN.tie_batch(name, width)], wide=True)
            assert None not in want


def test_alternation_across_seams(ctx):
    """denselib's alternation: an insertion run directly against a deletion run on every period -- two runs each time -- over
    21 strips of 64 columns."""
    sc, osc = scoring([2, -9, 0, -1])
    triples = [(*D.alternation(1300, 1300, k), w) for k, w in ((0, 3), (1, 40), (2, 600))]
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, triples, wide=True)
    assert None not in want and all(x[1] > 20 and x[2] > 20 for x in want), want


# ---------------------------------------------------------------- 7. errors, the time hook --
def test_errors_are_the_statistics_calls(ctx):
    """A band array of the wrong length, an unknown character pair inside the band: code and message as nw_stats_banded[_wide]."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    good = (b"ACGT" * 40, b"ACGT" * 40)
    pairs = [good] * 6
    pairs[4] = (good[0][:50] + b"X" + good[0][51:], good[1])
    batch = W.from_pairs(pairs)
    for gaps, stats in ((ctx.nw_gaps_banded, ctx.nw_stats_banded), (ctx.nw_gaps_banded_wide, ctx.nw_stats_banded_wide)):
        with pytest.raises(S.SeqAlignError) as ref:
            stats(batch, hyb, 5)
        with pytest.raises(S.SeqAlignError) as err:
            gaps(batch, hyb, 5)
        assert err.value.code == ref.value.code == S.E_UNKNOWN_PAIR and "pair 4:" in str(err.value)
        assert str(err.value).split(":", 1)[1] == str(ref.value).split(":", 1)[1]
        with pytest.raises(S.SeqAlignError) as err:
            gaps(batch, hyb, [5, 5])
        assert err.value.code == S.E_ARG


def test_the_band_time_hook(ctx):
    sc, _ = scoring(PLAIN)
    rng = random.Random(3)
    pairs = [(a, BL.mutate(rng, a, 0.05)) for a in (rand_seq(rng, 400) for _ in range(50))]
    ms = ctx.nw_gaps_band_time_ms(W.from_pairs(pairs), sc, 20, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms
