"""GPU tier: banded SW gap-run counts at any length -- seqalign_sw_gaps_banded and seqalign_sw_gaps_banded_wide
(sa_band_frame.hpp by sa_band_gaps.hip, sa_batch_band.hip).

Per pair (score, end_a, end_b, gap_runs_a, gap_runs_b) over the banded SW matrices: the banded score call's three byte for byte
and the numbers of maximal '-' runs in the two strings of the hit sw_align_banded(min_score = 1) delivers.  Every result the
oracle can hold is held to it (swgaplib.band_want: the banded hit, its strings counted) and to sw_score_banded(_wide); the wide
call returns the narrow call's bytes wherever that accepts the batch.  Past 65 535 letters the oracle still holds 66 000 x 180;
the pair of 66 000 x 65 960 is held to sw_align_banded_wide(min_score = 1)'s strings counted on the host.  No call may return the
hand-off time-out."""
import random

import numpy as np
import pytest

import bandlib as BL
import bandstatlib as BST
import bandspanlib as BSP
import bandswlib as BS
import bandswstatwidelib as BW
import orclib as O
import seqalign_amd as S
import spanlib as SP
import swgaplib as SG
import test_gpu_sw_stats_banded_wide as TW      # its shapes: geometry_cases, definition_pairs, busy_strips, scoring, run
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

PLAIN = TW.PLAIN
NARROW_MAX = 512
MIB = 1 << 20
N = SG.LONG


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def want_of(osc, pairs, lo, hi):
    """[(the banded score call's cell, the five values)] from the oracle."""
    return [SG.band_want(osc, a, b, lo[p], hi[p]) for p, (a, b) in enumerate(pairs)]


def check(ctx, sc, osc, pairs, lo, hi, want=None):
    """The wide call against the oracle, the wide score call (bytes) and, where the narrow call accepts the batch, the narrow
    call (bytes).  Returns the wanted list."""
    n = len(pairs)
    lo, hi = TW.per_pair(lo, n), TW.per_pair(hi, n)
    want = want or want_of(osc, pairs, lo, hi)
    batch = W.from_pairs(pairs)
    res = TW.run(ctx.sw_gaps_banded_wide, batch, sc, lo, hi)
    assert [r.dtype for r in res] == [np.int32] + [np.uint32] * 4 and all(r.shape == (n,) for r in res)
    got = SG.got_gaps(res)
    bad = [(p, len(pairs[p][0]), len(pairs[p][1]), lo[p], hi[p], got[p], want[p]) for p in range(n) if got[p] != want[p][1]]
    assert not bad, (len(bad), bad[:3])
    assert [w[0] for w in want] == [g[:3] for g in got]
    assert TW.same_bytes(res[:3], TW.run(ctx.sw_score_banded_wide, batch, sc, lo, hi))
    if all(BS.width_of(len(a), len(b), lo[p], hi[p]) <= NARROW_MAX for p, (a, b) in enumerate(pairs)):
        narrow = ctx.sw_gaps_banded(batch, sc, lo, hi)
        assert TW.same_bytes(res, narrow)
        assert TW.same_bytes(narrow[:3], ctx.sw_score_banded(batch, sc, lo, hi))
    return want


def n_hits(want):
    return sum(1 for cell, five in want if five[0] > 0)


# ---------------------------------------------------------------- 1. the definition --
@pytest.mark.parametrize("name", ["plain", "ext0", "ext_pos", "ext_pos2"])
def test_long_band_pairs(ctx, name):
    """bandswstatwidelib.long_band_pairs: bands left of, right of and across the main diagonal and empty ones, narrow and wide."""
    init, alpha = {"plain": (PLAIN, b"ACGT"), "ext0": ([3, -1, -1, 0], b"AC"), "ext_pos": ([2, -3, -2, 1], b"ACGT"),
                   "ext_pos2": ([3, -2, -3, 2], b"ACGT")}[name]
    sc, osc = TW.scoring(init)
    cases = BW.long_band_pairs(3200 + len(name), 120, alpha)
    pairs, lo, hi = [(a, b) for a, b, _, _ in cases], [c[2] for c in cases], [c[3] for c in cases]
    assert {BW.band_kind(len(a), len(b), l, h) for a, b, l, h in cases} == {"empty", "left", "right", "mid"}
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 40, n_hits(want)
    assert all(five == SG.ZEROS for (a, b, l, h), (cell, five) in zip(cases, want) if BS.clip(len(a), len(b), l, h) is None)


@pytest.mark.parametrize("name", list(TW.SW_SCORINGS))
def test_definition_dna_protein_and_no_mismatches(ctx, name):
    sc, osc, alphabet = TW.SW_SCORINGS[name]()
    pairs, lo, hi = TW.definition_pairs(random.Random(len(name) + 350), 48, alphabet)
    lo[0], hi[0] = 310, 350            # wholly right: empty after clipping for every len_a <= 300
    lo[1], hi[1] = -350, -5            # wholly left
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 16, n_hits(want)


def test_all_flag_combinations(ctx):
    import itertools

    import bandspanlib as BSP
    hits = 0
    with ctx.options(band_strip_cols=64):
        for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
            spec = BSP.flag_scoring(idx, flags)
            sc = S.make_scoring(spec)
            osc = O.Scoring.from_buffer_copy(bytes(sc))
            alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
            pairs, lo, hi = TW.definition_pairs(random.Random(7100 + idx), 8, alpha)
            hits += n_hits(check(ctx, sc, osc, pairs, lo, hi))
    assert hits >= 32 * 8 // 3, hits


def test_a_gap_that_pays_from_one_diagonal_outside_the_band(ctx):
    """gap_extend = +1: the walk steps onto a cell outside the band, which is a stop that has emitted no column -- a gap that
    extends out of it begins its run inside the band."""
    rng = random.Random(404)
    sc, osc = TW.scoring([2, -3, -2, 1])
    pairs, lo, hi = [], [], []
    for _ in range(40):
        read, window, offset = BS.read_in_window(rng, 150, 200, 0.08)
        pairs.append((TW.rand_seq(rng, 40) + read, window))
        lo.append(40 - offset - 4)
        hi.append(40 - offset + 4)
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, pairs, lo, hi)
    seven = [BST.want(osc, a, b, lo[p], hi[p])[1] for p, (a, b) in enumerate(pairs)]
    outside = [p for p, (a, b) in enumerate(pairs) if BSP.starts_outside(seven[p][:5], len(a), len(b), lo[p], hi[p])]
    assert len(outside) >= 10 and all(want[p][1][3] + want[p][1][4] > 0 for p in outside), len(outside)


NARROW_STEPS = (64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512)


def test_both_sides_of_every_step_of_the_narrow_ladder(ctx):
    """One pair of 290 letters, an indel relative, in bands of 64 .. 512 diagonals around the main one: 1 .. 6 and 8 diagonals
    per lane, both sides of every step."""
    sc, osc = TW.scoring(PLAIN)
    rng = random.Random(290)
    a = TW.rand_seq(rng, 290)
    b = SP.indel_relative(rng, a, b"ACGT")[:290]
    lo = [-(w // 2) for w in NARROW_STEPS]
    hi = [l + w - 1 for l, w in zip(lo, NARROW_STEPS)]
    pairs = [(a, b)] * len(NARROW_STEPS)
    assert [BS.width_of(len(a), len(b), l, h) for l, h in zip(lo, hi)] == list(NARROW_STEPS)
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert all(five[3] + five[4] > 0 for cell, five in want), want
    for p in range(len(pairs)):                                         # each width class in a launch of its own
        got = SG.got_gaps(ctx.sw_gaps_banded(W.from_pairs(pairs[p:p + 1]), sc, lo[p], hi[p]))
        assert got == [want[p][1]], (NARROW_STEPS[p], got, want[p])


@pytest.mark.parametrize("name", list(SP.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_across_seams(ctx, name):
    """bandstatlib.tie_batch at width 200 (4 strips of 64 columns): tie-dense pairs across the seams of narrow strips."""
    sc, osc = TW.scoring(SP.TIE_SCORINGS[name])
    pairs = BST.tie_batch(name, BST.TIE_WIDTHS[0])
    with ctx.options(band_strip_cols=64):
        for lo, hi in BST.TIE_BANDS:
            assert n_hits(check(ctx, sc, osc, pairs, lo, hi)) >= 30


# ---------------------------------------------------------------- 2. strip geometry, every strip width --
@pytest.fixture(scope="module")
def geometry(ctx):
    """test_gpu_sw_stats_banded_wide.py's 1 215 cases, the oracle's results and the narrow calls' (computed once)."""
    pairs, lo, hi = TW.geometry_cases()
    sc, osc = TW.scoring(PLAIN)
    want = want_of(osc, pairs, lo, hi)
    assert n_hits(want) >= 400
    batch = W.from_pairs(pairs)
    narrow = ctx.sw_gaps_banded(batch, sc, lo, hi)
    assert SG.got_gaps(narrow) == [w[1] for w in want]
    assert TW.same_bytes(narrow[:3], ctx.sw_score_banded(batch, sc, lo, hi))
    return dict(lo=lo, hi=hi, sc=sc, batch=batch, narrow=narrow)


@pytest.mark.parametrize("cols", [64, 128, 256, 512, 0])
def test_strip_geometry_at_every_strip_width(ctx, geometry, cols):
    g = geometry
    with ctx.options(band_strip_cols=cols):
        res = TW.run(ctx.sw_gaps_banded_wide, g["batch"], g["sc"], g["lo"], g["hi"])
    assert TW.same_bytes(res, g["narrow"])


@pytest.mark.parametrize("cols", [64, 128, 256, 512, 0])
def test_widths_513_and_1025(ctx, cols):
    """One pair of 2 600 letters at 513, 1 025 and 1 401 diagonals: the narrow call refuses each, the wide call equals the oracle
    and the '-' runs of the GPU's own align call's strings."""
    sc, osc = TW.scoring(PLAIN)
    rng = random.Random(2600)
    a, b = TW.related(rng, 2600, 0.08)
    b = (TW.rand_seq(rng, 40) + b)[:2600]
    pairs, lo, hi = [(a, b)] * 3, [-256, -512, -700], [256, 512, 700]
    assert [BS.width_of(2600, len(b), l, h) for l, h in zip(lo, hi)] == [513, 1025, 1401]
    for p in range(3):
        with pytest.raises(S.SeqAlignError) as e:
            ctx.sw_gaps_banded(W.from_pairs(pairs[:1]), sc, lo[p], hi[p])
        assert e.value.code == S.E_TOO_LARGE and "pair 0:" in str(e.value) and "diagonals" in str(e.value)
    with ctx.options(band_strip_cols=cols):
        want = check(ctx, sc, osc, pairs, lo, hi)
        hits = TW.run(ctx.sw_align_banded_wide, W.from_pairs(pairs), sc, lo, hi, 1)
    assert [w[1] for w in want] == [SG.host_gaps(h) for h in hits]
    assert all(five[3] > 0 and five[4] > 0 for cell, five in want), want


# ---------------------------------------------------------------- 3. bytes, budget, accounting, errors --
def model_bytes(la, lb, lo, hi, cols=64):
    """The contract's device bytes of one pair: the span call's (an empty band is handed to the kernel as one diagonal)."""
    strips = max(1, -(-la // cols))
    return la + lb + 88 + strips * (32 * max(1, BS.width_of(la, lb, lo, hi)) + 36) + 20


def test_a_pair_over_the_budget_is_nomem_with_the_bytes_named(ctx):
    sc, _ = TW.scoring(PLAIN)
    rng = random.Random(7000)
    a = TW.rand_seq(rng, 320)
    b = (TW.rand_seq(rng, 3000) + BL.mutate(rng, a, 0.05) + TW.rand_seq(rng, 7000))[:7000]
    small = (TW.rand_seq(rng, 70), TW.rand_seq(rng, 66))
    batch, lo, hi = W.from_pairs([small, (a, b), small]), [-3, -7000, -3], [3, 320, 3]
    need = model_bytes(320, 7000, -7000, 320)
    assert need == 320 + 7000 + 88 + 5 * (32 * 7321 + 36) + 20 and need - 1 >= MIB
    with ctx.options(band_strip_cols=64):
        with ctx.options(chunk_bytes=need):
            got = TW.run(ctx.sw_gaps_banded_wide, batch, sc, lo, hi)
            assert ctx.last_call()["band_score"][0] == 3                # each pair a chunk of its own
            span = TW.run(ctx.sw_span_banded_wide, batch, sc, lo, hi)   # the same bytes per pair: the same cut
            assert ctx.last_call()["band_score"][0] == 3
        assert np.array_equal(got[0], span[0]) and np.array_equal(got[1], span[1] + span[3])
        full = ctx.sw_gaps(W.from_pairs([(a, b)]), sc)               # the whole matrix as the band: the unbanded call
        assert [int(x[1]) for x in got] == [int(x[0]) for x in full]
        for fn in (ctx.sw_gaps_banded_wide, ctx.sw_span_banded_wide):
            with ctx.options(chunk_bytes=need - 1):
                with pytest.raises(S.SeqAlignError) as e:
                    TW.run(fn, batch, sc, lo, hi)
            assert e.value.code == S.E_NOMEM and "pair 1:" in str(e.value) and f" {need} bytes" in str(e.value), str(e.value)


def test_accounting_under_band_score(ctx):
    sc, _ = TW.scoring(PLAIN)
    rng = random.Random(11)
    pairs = [TW.related(rng, n) for n in (0, 30, 64, 65, 200, 640, 700)] + [(TW.rand_seq(rng, 100), b""), (b"", TW.rand_seq(rng, 9))]
    batch = W.from_pairs(pairs)
    for cols in (64, 256):
        for lo, hi in ((-10, 10), (100, 330), (650, 660)):
            busy = sum(TW.busy_strips(len(a), len(b), lo, hi, cols) for a, b in pairs)
            with ctx.options(band_strip_cols=cols):
                TW.run(ctx.sw_gaps_banded_wide, batch, sc, lo, hi)
            assert ctx.last_call() == {"band_score": (1, busy)}, (cols, lo, hi, ctx.last_call(), busy)
    ctx.sw_gaps_banded(batch, sc, -10, 10)
    ran = ctx.last_call()
    assert set(ran) == {"band_score"} and ran["band_score"][1] == len(pairs), ran      # one launch per width class, items: pairs
    ms = ctx.sw_gaps_band_time_ms(batch, sc, -10, 10, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms


def test_errors_are_the_span_calls(ctx):
    """diag_lo > diag_hi, the width cap of the narrow call, an unknown character pair inside the band only: status and message of
    sw_span_banded(_wide) on the same arguments; sequences over 65 535 letters are taken."""
    sc, _ = TW.scoring(PLAIN)
    rng = random.Random(8)
    short = (TW.rand_seq(rng, 50), TW.rand_seq(rng, 60))
    long_ = (TW.rand_seq(rng, N, b"AC"), TW.rand_seq(rng, 20, b"GT"))
    square = (TW.rand_seq(rng, 700), TW.rand_seq(rng, 700))
    for pairs, lo, hi in (([short, short], [-3, 4], [3, 3]), ([long_, short, short], [-3, -3, 9], [3, 3, 8]), ([short, square], -300, 300)):
        for fn, ref in ((ctx.sw_gaps_banded_wide, ctx.sw_span_banded_wide), (ctx.sw_gaps_banded, ctx.sw_span_banded)):
            if fn == ctx.sw_gaps_banded_wide and np.isscalar(lo):
                continue                                        # (601 diagonals: legal in the wide call)
            with pytest.raises(S.SeqAlignError) as want:
                ref(W.from_pairs(pairs), sc, lo, hi)
            with pytest.raises(S.SeqAlignError) as got:
                TW.run(fn, W.from_pairs(pairs), sc, lo, hi)
            assert got.value.code == want.value.code
            assert str(got.value).replace("sw_gaps", "sw_span") == str(want.value), (str(got.value), str(want.value))
    with ctx.options(band_strip_cols=64):
        res = TW.run(ctx.sw_gaps_banded_wide, W.from_pairs([short, long_]), sc, -300, 300)
    assert SG.got_gaps(res)[1] == SG.ZEROS
    hyb = S.make_scoring({"preset": "DNA_hybridization",
                          "mutations": [["x", c, -1] for c in "acgt"] + [[c, "y", -1] for c in "acgt"]})
    a = b"ACGGTCATTG" * 60
    b = a[:290] + b"T" + a[290:]
    with_x = a[:300] + b"X" + a[301:]
    near, far = b[:302] + b"Y" + b[303:], b[:20] + b"Y" + b[21:]
    inside = W.from_pairs([(a, b), (with_x, far), (with_x, near), (a, b)])
    with ctx.options(band_strip_cols=64):
        for fn, ref in ((ctx.sw_gaps_banded_wide, ctx.sw_span_banded_wide), (ctx.sw_gaps_banded, ctx.sw_span_banded)):
            with pytest.raises(S.SeqAlignError) as want:
                ref(inside, hyb, -8, 8)
            with pytest.raises(S.SeqAlignError) as got:
                TW.run(fn, inside, hyb, -8, 8)
            assert got.value.code == S.E_UNKNOWN_PAIR and "pair 2:" in str(got.value)
            assert str(got.value).replace("sw_gaps", "sw_span") == str(want.value)
        ok = TW.run(ctx.sw_gaps_banded_wide, W.from_pairs([(a, b), (with_x, far)]), hyb, -8, 8)      # X against Y outside the band
    assert int(ok[0][1]) > 0


# ---------------------------------------------------------------- 4. past 65 535 letters --
def long_pair(case):
    """A long sequence of 66 000 letters and a short one of 180 with a hit of about 120 letters at columns / rows 65 700 ..
    65 820 of the long one -- two letters of it missing from the short one and two others inserted there -- in 600 diagonals.
    "a": len_a = 66 000: 1 032 strips of 64 columns, the last frames overhang len_a.  "b": len_b = 66 000, 3 strips."""
    rng = random.Random(66 + len(case))
    core = bytes(rng.choice(b"GT") for _ in range(120))
    core2 = core[:40] + core[42:80] + b"KM" + core[80:]
    long_ = bytearray(rng.choice(b"AC") for _ in range(N))
    short = bytearray(rng.choice(b"KM") for _ in range(180))
    long_[65700:65820] = core
    short[40:160] = core2
    if case == "a":
        return (bytes(long_), bytes(short)), 65250, 65849
    return (bytes(short), bytes(long_)), -65999, -65400


@pytest.mark.parametrize("case", ["a", "b"])
def test_a_gapped_hit_past_coordinate_65535_in_600_diagonals(ctx, case):
    sc, osc = TW.scoring(PLAIN)
    (a, b), lo, hi = long_pair(case)
    assert max(len(a), len(b)) == N and BS.width_of(len(a), len(b), lo, hi) == 600
    batch = W.from_pairs([(a, b)])
    with pytest.raises(S.SeqAlignError) as e:                         # the width cap of the narrow call
        ctx.sw_gaps_banded(batch, sc, lo, hi)
    assert e.value.code == S.E_TOO_LARGE
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, [(a, b)], lo, hi)
    score, end_a, end_b, ga, gb = want[0][1]
    assert score > 150 and (ga, gb) == (1, 1) and (end_a if case == "a" else end_b) == 65820, want


@pytest.fixture(scope="module")
def constructed():
    return SG.deleted_block(W.Rng(66000))


@pytest.mark.parametrize("geom", ["narrow 80", "wide 300 / 64", "wide 300 / 512"])
def test_deleted_block_past_65535_across_every_seam(ctx, constructed, geom):
    """66 000 x 65 960, a sequence against itself with one block of 40 deleted: the hit crosses every strip seam and the run
    lies past none of the 16-bit limits' reach.  Held to sw_align_banded_wide(min_score = 1)'s strings counted on the host."""
    sc, osc = TW.scoring(SG.BLOCK_INIT)
    batch = W.from_pairs([constructed])
    w = 80 if geom == "narrow 80" else 300
    with ctx.options(band_strip_cols=512 if geom.endswith("512") else 64):
        fn = ctx.sw_gaps_banded if geom == "narrow 80" else ctx.sw_gaps_banded_wide
        got = SG.got_gaps(TW.run(fn, batch, sc, -w, w))[0]
        score = TW.run(ctx.sw_score_banded_wide, batch, sc, -w, w)
        assert tuple(int(x[0]) for x in score) == got[:3]
        hits, = TW.run(ctx.sw_align_banded_wide, batch, sc, -w, w, 1)
    assert SG.host_gaps(hits) == got, (SG.host_gaps(hits), got)
    assert got[1:] == (N, N - 40, 0, 1), got
