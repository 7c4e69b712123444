"""GPU tier: the wide banded calls -- seqalign_{nw,sw}_{score,align}_banded_wide (sa_band_strips.hip, sa_batch_band.hip).

The four contracts are the narrow calls' at any width: results are checked against the Python definitions (bandlib,
bandswlib), against the narrow calls byte for byte wherever those accept the batch, and across every strip width.  Unless
stated the strips are forced to 64 columns (option band_strip_cols), so that small pairs have several strips.  No call may
return the hand-off time-out."""
import itertools
import json
import random
from pathlib import Path

import numpy as np
import pytest

import bandlib as BL
import bandswlib as BS
import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

FULL = 2 ** 31
PLAIN = [1, -2, -4, -1]
SW_PLAIN = [2, -3, -4, -1]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def scoring(init, **more):
    sc = S.make_scoring({"init": [*init, *([0] * (10 - len(init)))], **more})
    return sc, O.Scoring.from_buffer_copy(bytes(sc))


def run(fn, *args):
    """fn(*args); an error passes through, but never the hand-off time-out."""
    try:
        return fn(*args)
    except S.SeqAlignError as e:
        assert "timed out" not in str(e), str(e)
        raise


def nw_both(ctx, batch, sc, band):
    """The wide align call's result, after checking that the wide score call agrees with it."""
    got = run(ctx.nw_align_banded_wide, batch, sc, band)
    score = run(ctx.nw_score_banded_wide, batch, sc, band)
    assert [g[0] for g in got] == [int(s) for s in score]
    return got


def sw_both(ctx, batch, sc, lo, hi, min_score=1):
    """(score cells, hits) of the two wide SW calls."""
    score, end_a, end_b = run(ctx.sw_score_banded_wide, batch, sc, lo, hi)
    cells = [(int(score[p]), int(end_a[p]), int(end_b[p])) for p in range(batch.n_pairs)]
    return cells, run(ctx.sw_align_banded_wide, batch, sc, lo, hi, min_score)


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def related(rng, n, edits=0.05, tail=0, alphabet=b"ACGT"):
    a = rand_seq(rng, n, alphabet)
    b = BL.mutate(rng, a, edits, alphabet)
    return (a + rand_seq(rng, tail, alphabet), b) if tail > 0 else (a, b + rand_seq(rng, -tail, alphabet))


# ---------------------------------------------------------------- 1. the definition, NW --
def test_definition_nw_all_flag_combinations(ctx):
    rng = random.Random(1501)
    n_none = 0
    with ctx.options(band_strip_cols=64):
        for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
            both_no_gaps = flags[2] and flags[3]
            init = [1, -6 if both_no_gaps else -2, -4, -1] if idx % 2 else [2, -7 if both_no_gaps else -3, 0, -2]
            sc, osc = scoring([*init, *flags])
            pairs, bands = [], []
            for k in range(8):
                la = rng.randrange(0, 301)
                a = rand_seq(rng, la, b"ACGTacgt")
                b = BL.mutate(rng, a, 0.2, b"ACGTacgt")[:300] if rng.random() < 0.7 else rand_seq(rng, rng.randrange(0, 301), b"ACGTacgt")
                pairs.append((a, b))
                bands.append(150 if (idx + k) % 11 == 0 else rng.randrange(0, 41))
            both = [BL.expected_both(osc, a, b, w) for (a, b), w in zip(pairs, bands)]
            want_score, want = [x[0] for x in both], [x[1] for x in both]
            batch = W.from_pairs(pairs)
            assert [int(s) for s in run(ctx.nw_score_banded_wide, batch, sc, bands)] == want_score, (flags, init)
            none = [p for p, x in enumerate(want) if x is None]
            n_none += len(none)
            if none:
                with pytest.raises(S.SeqAlignError) as e:
                    run(ctx.nw_align_banded_wide, batch, sc, bands)
                assert e.value.code == S.E_TRACEBACK and f"pair {none[0]}:" in str(e.value), (str(e.value), none)
                keep = [p for p in range(len(pairs)) if want[p] is not None]
                pairs, bands, want = [pairs[p] for p in keep], [bands[p] for p in keep], [want[p] for p in keep]
                batch = W.from_pairs(pairs)
            got = nw_both(ctx, batch, sc, bands)
            bad = [(p, len(pairs[p][0]), len(pairs[p][1]), bands[p], got[p][0], want[p][0]) for p in range(len(pairs)) if got[p] != want[p]]
            assert not bad, (flags, init, bad[:3])
    assert n_none > 0


# ---------------------------------------------------------------- 2. strip geometry, NW --
def geometry_cases():
    rng = random.Random(64)
    pairs, bands = [], []
    for la in (1, 63, 64, 65, 127, 128, 129, 192, 257):
        a = rand_seq(rng, la)
        for delta in (-70, -1, 0, 1, 70):
            lb = max(0, la + delta)
            b = (BL.mutate(rng, a, 0.1) + rand_seq(rng, lb))[:lb]
            for w in (0, 1, 31, 32, 33, 63, 64, 65, 100):
                pairs.append((a, b))
                bands.append(w)
    return pairs, bands


@pytest.fixture(scope="module")
def geometry(ctx):
    """The cases, bandlib's results, and the narrow calls' (computed once)."""
    pairs, bands = geometry_cases()
    sc, osc = scoring(PLAIN)
    want = [BL.expected(osc, a, b, w) for (a, b), w in zip(pairs, bands)]
    batch = W.from_pairs(pairs)
    return dict(pairs=pairs, bands=bands, sc=sc, want=want, batch=batch, narrow=ctx.nw_align_banded(batch, sc, bands),
                narrow_score=ctx.nw_score_banded(batch, sc, bands))


def test_strip_geometry_nw(ctx, geometry):
    g = geometry
    assert len(g["pairs"]) == 405 and all(x is not None for x in g["want"])
    with ctx.options(band_strip_cols=64):
        got = run(ctx.nw_align_banded_wide, g["batch"], g["sc"], g["bands"])
        score = run(ctx.nw_score_banded_wide, g["batch"], g["sc"], g["bands"])
    bad = [(p, len(g["pairs"][p][0]), len(g["pairs"][p][1]), g["bands"][p]) for p in range(len(got)) if got[p] != g["want"][p]]
    assert not bad, bad[:5]
    assert got == g["narrow"]
    assert score.tobytes() == g["narrow_score"].tobytes()


# ---------------------------------------------------------------- 3. every strip width --
@pytest.mark.parametrize("cols", [64, 128, 256, 512, 0])
def test_every_strip_width(ctx, geometry, cols):
    g = geometry
    pick = sorted({(k * 404) // 59 for k in range(60)})
    assert len(pick) == 60
    pairs, bands = [g["pairs"][p] for p in pick], [g["bands"][p] for p in pick]
    batch = W.from_pairs(pairs)
    with ctx.options(band_strip_cols=cols):
        got = nw_both(ctx, batch, g["sc"], bands)
    assert got == [g["want"][p] for p in pick] == [g["narrow"][p] for p in pick]


# ---------------------------------------------------------------- 4. past 1 024, NW --
def past_1024_nw():
    rng = random.Random(1025)
    cases = []
    a, b = related(rng, 1300, 0.03)
    cases.append((a, (b + rand_seq(rng, 100))[:1308], 512))
    a, b = related(rng, 2600, 0.05)
    cases.append((a, (b + rand_seq(rng, 200))[:2600], 1024))
    a, b = related(rng, 2600, 0.05)
    cases.append((a, (b + rand_seq(rng, 200))[:2590], 1500))
    a, b = related(rng, 2600, 0.05)
    cases.append((a, b[:1500], 600))
    a, b = related(rng, 900, 0.05)
    b = (b + rand_seq(rng, 100))[:880]
    cases.append((a, b, BL.w_for_width(900, 880, 1025)))
    return cases


@pytest.fixture(scope="module")
def wide_nw():
    sc, osc = scoring(PLAIN)
    cases = past_1024_nw()
    widths = [BL.width_of(len(a), len(b), w) for a, b, w in cases]
    assert widths[4] == 1025 and 1025 <= widths[0] <= 1045 and 2040 <= widths[1] <= 2060 and 3005 <= widths[2] <= 3020, widths
    assert all(x > 1024 for x in widths)
    return sc, cases, [BL.expected(osc, a, b, w) for a, b, w in cases]


@pytest.mark.parametrize("cols", [0, 64, 512])
def test_past_1024_nw(ctx, wide_nw, cols):
    sc, cases, want = wide_nw
    batch = W.from_pairs([(a, b) for a, b, _ in cases])
    bands = [w for _, _, w in cases]
    with pytest.raises(S.SeqAlignError) as e:
        ctx.nw_score_banded(batch, sc, bands)                  # the narrow calls refuse these
    assert e.value.code == S.E_TOO_LARGE
    with ctx.options(band_strip_cols=cols):
        assert nw_both(ctx, batch, sc, bands) == want
        # a band that covers the whole matrix
        rng = random.Random(79)
        a, b = related(rng, 700, 0.1)
        whole = W.from_pairs([(a, (b + rand_seq(rng, 300))[:900])])
        got = nw_both(ctx, whole, sc, FULL)
    assert got == ctx.nw_batch(whole, sc)
    assert [g[0] for g in got] == [int(s) for s in ctx.nw_score(whole, sc)]


# ---------------------------------------------------------------- 5. the definition, SW --
def _protein():
    presets = json.loads((Path(__file__).resolve().parent / "golden" / "presets.json").read_text())
    sc = S.make_scoring({"preset": "BLOSUM62"})
    assert bytes(O.build_scoring(presets["BLOSUM62"]["spec"]))[:8] == bytes(sc)[:8]
    return sc, O.Scoring.from_buffer_copy(bytes(sc)), b"ARNDCQEGHILKMFPSTWYV"


SW_SCORINGS = {
    "plain": lambda: (*scoring(SW_PLAIN), b"ACGT"),
    "no_mismatches": lambda: (*scoring([2, -3, -4, -1, 0, 0, 0, 0, 1]), b"ACGT"),
    "BLOSUM62": _protein,
}


@pytest.mark.parametrize("name", list(SW_SCORINGS))
def test_definition_sw(ctx, name):
    sc, osc, alphabet = SW_SCORINGS[name]()
    rng = random.Random(len(name) + 350)
    pairs, lo, hi = [], [], []
    for k in range(48):
        la = rng.randrange(0, 301)
        a = rand_seq(rng, la, alphabet)
        if rng.random() < 0.7:
            core = BL.mutate(rng, a, 0.15, alphabet)
            b = (rand_seq(rng, rng.randrange(0, 80), alphabet) + core)[:300]
        else:
            b = rand_seq(rng, rng.randrange(0, 301), alphabet)
        x, y = rng.randrange(-350, 351), rng.randrange(-350, 351)
        pairs.append((a, b))
        lo.append(min(x, y))
        hi.append(max(x, y))
    lo[0], hi[0] = 310, 350            # wholly right: empty after clipping for every len_a <= 300
    lo[1], hi[1] = -350, -5            # wholly left
    batch = W.from_pairs(pairs)
    kinds = {("empty" if BS.clip(len(a), len(b), l, h) is None else "left" if h < 0 else "right" if l > 64 else "mid")
             for (a, b), l, h in zip(pairs, lo, hi)}
    assert kinds == {"empty", "left", "right", "mid"}, kinds
    for min_score in (1, 20):
        want = [BS.expected(osc, a, b, lo[p], hi[p], min_score) for p, (a, b) in enumerate(pairs)]
        with ctx.options(band_strip_cols=64):
            cells, hits = sw_both(ctx, batch, sc, lo, hi, min_score)
        bad = [(p, len(pairs[p][0]), len(pairs[p][1]), lo[p], hi[p], cells[p], want[p][0]) for p in range(48) if cells[p] != want[p][0]]
        assert not bad, ("score call", bad[:3])
        bad = [(p, lo[p], hi[p], hits[p], want[p][1]) for p in range(48) if hits[p] != ([want[p][1]] if want[p][1] else [])]
        assert not bad, ("align call", bad[:2])
        narrow = ctx.sw_score_banded(batch, sc, lo, hi)
        assert cells == [(int(narrow[0][p]), int(narrow[1][p]), int(narrow[2][p])) for p in range(48)]
        assert hits == ctx.sw_align_banded(batch, sc, lo, hi, min_score)
    assert sum(1 for c, h in want if c[0] > 0) >= 16


# ---------------------------------------------------------------- 6. ties across strips, SW --
def test_ties_across_strips_sw(ctx):
    sc, osc = scoring(SW_PLAIN)
    unit = rand_seq(random.Random(6), 40)
    for a, b in ((unit * 6, unit), (unit, unit * 6)):
        la, lb = len(a), len(b)
        batch = W.from_pairs([(a, b)])
        full = ctx.sw_batch(batch, sc, 1, max_hits=1)
        for lo, hi in ((-lb, la), (-FULL, FULL - 1), (45, la), (-lb, 100), (-130, -50), (70, 170), (-lb, -15)):
            if lo > hi:                                # (45, la) on the 40-letter seq_a
                continue
            want = BS.expected(osc, a, b, lo, hi)
            with ctx.options(band_strip_cols=64):
                cells, hits = sw_both(ctx, batch, sc, lo, hi)
            assert cells == [want[0]] and hits == [[want[1]] if want[1] else []], (la, lb, lo, hi, cells, want[0])
            if lo <= -lb and hi >= la:
                assert hits == full and cells[0] == (80, 40, 40)


# ---------------------------------------------------------------- 7. past 1 024, SW --
@pytest.fixture(scope="module")
def wide_sw():
    sc, osc = scoring(SW_PLAIN)
    rng = random.Random(2600)
    a, b = related(rng, 2600, 0.08)
    b = (rand_seq(rng, 40) + b)[:2600]
    c = rand_seq(rng, 2600)
    d = BL.mutate(rng, c[900:1900], 0.08) + rand_seq(rng, 200)          # lies along diagonals near +900
    cases = [(a, b, -700, 700), (c, d[:1200], 500, 1700)]
    return sc, cases, [BS.expected(osc, *case) for case in cases]


@pytest.mark.parametrize("cols", [0, 64])
def test_past_1024_sw(ctx, wide_sw, cols):
    sc, cases, want = wide_sw
    assert all(BS.width_of(len(a), len(b), lo, hi) > 1024 for a, b, lo, hi in cases) and all(w[0][0] > 100 for w in want)
    batch = W.from_pairs([(a, b) for a, b, _, _ in cases])
    lo, hi = [c[2] for c in cases], [c[3] for c in cases]
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_score_banded(batch, sc, lo, hi)
    assert e.value.code == S.E_TOO_LARGE
    with ctx.options(band_strip_cols=cols):
        cells, hits = sw_both(ctx, batch, sc, lo, hi)
    assert cells == [w[0] for w in want]
    assert hits == [[w[1]] for w in want]


# ---------------------------------------------------------------- 8. mixed batch and chunks --
def test_mixed_batch_and_chunks(ctx):
    sc, _ = scoring(PLAIN)
    ssc, _ = scoring(SW_PLAIN)
    rng = random.Random(88)
    # strips of 64 columns: len_a = 0 -> none busy, 1 .. 64 -> 1, 65 .. 128 -> 2, 257 .. 320 -> 5, 2 561 .. 2 624 -> 41
    shape = [(0, 30, 5), (40, 44, 0), (64, 60, 10), (100, 100, 0), (128, 90, 30), (300, 310, 16), (320, 300, 200), (2600, 400, 400),
             (2624, 2600, 40), (1, 1, 0), (300, 0, 0), (50, 50, FULL), (65, 64, 1), (2570, 2600, 300), (127, 127, 63), (290, 257, 2),
             (30, 0, 0), (0, 0, 0), (310, 310, 33), (90, 128, 7), (2561, 2561, 100)]
    assert len(shape) == 21
    pairs = []
    for la, lb, _ in shape:
        a = rand_seq(rng, la)
        pairs.append((a, (BL.mutate(rng, a, 0.05) + rand_seq(rng, lb))[:lb]))
    bands = [w for _, _, w in shape]
    strips = {max(1, -(-la // 64)) if la else 0 for la, _, _ in shape}
    widths = [BL.width_of(la, lb, w) for la, lb, w in shape]
    assert {0, 1, 2, 5, 41} <= strips and min(widths) == 1 and 2990 <= max(widths) <= 3010, (strips, min(widths), max(widths))
    batch = W.from_pairs(pairs)
    lo = [-min(w, 2000) - 3 for w in bands]
    hi = [min(w, 2000) + 5 for w in bands]
    with ctx.options(band_strip_cols=64):
        nw = nw_both(ctx, batch, sc, bands)
        sw_cells, sw_hits = sw_both(ctx, batch, ssc, lo, hi, 10)
        for p in range(21):
            one = W.from_pairs([pairs[p]])
            assert nw_both(ctx, one, sc, bands[p]) == [nw[p]], p
            c1, h1 = sw_both(ctx, one, ssc, lo[p], hi[p], 10)
            assert c1 == [sw_cells[p]] and h1 == [sw_hits[p]], p
        with ctx.options(chunk_bytes=22 << 20):        # the largest pair alone needs 12 x 2 601 x 631 bytes of cells
            assert run(ctx.nw_align_banded_wide, batch, sc, bands) == nw
            info = ctx.last_call()
            assert info["band_fill"][0] >= 3 and info["band_walk"][0] == info["band_fill"][0], info
            assert run(ctx.sw_align_banded_wide, batch, ssc, lo, hi, 10) == sw_hits
            assert ctx.last_call()["band_fill"][0] >= 3


# ---------------------------------------------------------------- 9. errors --
def test_errors(ctx):
    """X (in seq_a) against Y (in seq_b) has no score; every other pair of letters has one."""
    sc = S.make_scoring({"preset": "DNA_hybridization",
                         "mutations": [["x", c, -1] for c in "acgt"] + [[c, "y", -1] for c in "acgt"]})
    a = b"ACGGTCATTG" * 60
    b = a[:290] + b"T" + a[290:]
    with_x = a[:300] + b"X" + a[301:]              # column 301: the fifth strip of 64
    near = b[:302] + b"Y" + b[303:]                # row 303 against column 301: diagonal -2
    far = b[:20] + b"Y" + b[21:]                   # row 21 against column 301: diagonal 280
    good = (a, b)
    inside = W.from_pairs([good, good, (with_x, far), (with_x, near), good, (with_x, near)])
    outside = W.from_pairs([good, (with_x, far), good])
    with ctx.options(band_strip_cols=64):
        for call, narrow in ((ctx.nw_score_banded_wide, ctx.nw_score_banded), (ctx.nw_align_banded_wide, ctx.nw_align_banded)):
            with pytest.raises(S.SeqAlignError) as want:
                narrow(inside, sc, 8)
            with pytest.raises(S.SeqAlignError) as got:
                run(call, inside, sc, 8)
            assert got.value.code == S.E_UNKNOWN_PAIR and "pair 3:" in str(got.value), str(got.value)
            assert str(got.value).split("] ")[-1] == str(want.value).split("] ")[-1]
        got = nw_both(ctx, outside, sc, 8)
        assert got == ctx.nw_align_banded(outside, sc, 8)
        assert got[0] == got[2] and got[1][1].replace(b"-", b"") == with_x
        for call, tail in ((ctx.sw_score_banded_wide, ()), (ctx.sw_align_banded_wide, (1,))):
            with pytest.raises(S.SeqAlignError) as got:
                run(call, inside, sc, -8, 8, *tail)
            assert got.value.code == S.E_UNKNOWN_PAIR and "pair 3:" in str(got.value), str(got.value)
            run(call, outside, sc, -8, 8, *tail)
        # a pair larger than the chunk budget
        plain, _ = scoring(PLAIN)
        rng = random.Random(9)
        big = W.from_pairs([related(rng, 600), related(rng, 2400), related(rng, 600)])
        with ctx.options(chunk_bytes=1 << 20):
            with pytest.raises(S.SeqAlignError) as e:
                run(ctx.nw_align_banded_wide, big, plain, [20, 100, 20])
            assert e.value.code == S.E_NOMEM and "pair 1:" in str(e.value) and "bytes" in str(e.value), str(e.value)
            digits = [int(t) for t in str(e.value).replace(",", " ").split() if t.isdigit()]
            assert any(d >= 12 * 2300 * 201 for d in digits), str(e.value)      # the bytes needed are named
            with pytest.raises(S.SeqAlignError) as e:
                run(ctx.sw_align_banded_wide, big, plain, [-20, -100, -20], [20, 100, 20], 1)
            assert e.value.code == S.E_NOMEM and "pair 1:" in str(e.value) and "bytes" in str(e.value), str(e.value)


# ---------------------------------------------------------------- 10. off the fast path --
@pytest.mark.parametrize("init", [[5, -4, 3, -4], [3, -2, -5, 1], [1, -2, -4, -1, 1, 1]], ids=["gap_open+", "gap_extend+", "free_ends"])
def test_off_the_fast_path(ctx, init):
    sc, osc = scoring(init)
    rng = random.Random(65)
    pairs, bands = [], []
    for lb in (65, 129, 193):                      # one past a multiple of 64; len_a = 65: the last column alone in its strip
        a = rand_seq(rng, 65)
        for w in (0, 3, 40, 64, 200):
            pairs.append((a, (BL.mutate(rng, a, 0.1) + rand_seq(rng, lb))[:lb]))
            bands.append(w)
    want = [BL.expected_both(osc, a, b, w) for (a, b), w in zip(pairs, bands)]
    batch = W.from_pairs(pairs)
    with ctx.options(band_strip_cols=64):
        assert [int(s) for s in run(ctx.nw_score_banded_wide, batch, sc, bands)] == [x[0] for x in want]
        assert all(x[1] is not None for x in want)
        assert run(ctx.nw_align_banded_wide, batch, sc, bands) == [x[1] for x in want]
    assert ctx.nw_align_banded(batch, sc, bands) == [x[1] for x in want]


# ---------------------------------------------------------------- 11. what ran --
def test_accounting(ctx):
    sc, _ = scoring(PLAIN)
    ssc, _ = scoring(SW_PLAIN)
    rng = random.Random(11)
    pairs = [related(rng, n) for n in (0, 30, 64, 65, 200, 640, 700)] + [(rand_seq(rng, 100), b"")]
    batch = W.from_pairs(pairs)
    n = batch.n_pairs
    for cols in (64, 256):
        ceil = lambda x: -(-x // cols)
        with ctx.options(band_strip_cols=cols):
            # NW: every column of a pair with rows has an inner band cell
            cols_nw = [len(a) if len(b) else 0 for a, b in pairs]
            low = sum(ceil(x) for x in cols_nw)
            run(ctx.nw_score_banded_wide, batch, sc, 10)
            info = ctx.last_call()
            assert set(info) == {"band_score"} and info["band_score"][0] == 1 and low <= info["band_score"][1] <= low + n, info
            run(ctx.nw_align_banded_wide, batch, sc, 10)
            info = ctx.last_call()
            assert set(info) == {"band_fill", "band_walk"} and info["band_walk"] == (1, n), info
            assert info["band_fill"][0] == 1 and low <= info["band_fill"][1] <= low + n, info
            # SW: the columns max(1, 1 + d_lo) .. min(len_a, len_b + d_hi)
            lo, hi = 70, 90
            cols_sw = []
            for a, b in pairs:
                band = BS.clip(len(a), len(b), lo, hi)
                cols_sw.append(0 if band is None or not len(b) else max(0, min(len(a), len(b) + band[1]) - max(1, 1 + band[0]) + 1))
            low = sum(ceil(x) for x in cols_sw)
            assert low > 0
            run(ctx.sw_score_banded_wide, batch, ssc, lo, hi)
            info = ctx.last_call()
            assert set(info) == {"band_score"} and low <= info["band_score"][1] <= low + n, (info, low)
            run(ctx.sw_align_banded_wide, batch, ssc, lo, hi, 1)
            info = ctx.last_call()
            assert set(info) == {"band_fill", "band_walk"} and low <= info["band_fill"][1] <= low + n, (info, low)
