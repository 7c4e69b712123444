"""GPU tier: wide banded SW hit spans -- seqalign_sw_span_banded_wide (sa_band_frame.hpp by sa_band_span.hip, sa_batch_band.hip).

The contract is seqalign_sw_span_banded's at any clipped width and any length.  Every result is checked bit for bit against the
oracle (bandspanlib.want: the five fields of the banded hit, zeros without one), the first three (score, pos + len) against
ctx.sw_score_banded_wide, all five arrays byte for byte against ctx.sw_span_banded wherever the narrow call accepts the batch
(width <= 512), and against the first five of ctx.sw_stats_banded_wide wherever that call accepts it (at most 65 535 letters).
Unless stated the strips are forced to 64 columns (option band_strip_cols), so that pairs of at most 300 letters have several
strips.  No call may return the hand-off time-out."""
import itertools
import json
import random
from pathlib import Path

import numpy as np
import pytest

import bandlib as BL
import bandspanlib as BSP
import bandspanwidelib as BW
import bandswlib as BS
import maglib as G
import orclib as O
import seqalign_amd as S
import spanlib as SP
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

PLAIN = [2, -3, -4, -1]
FULL = 2 ** 31
NARROW_MAX = 512
STATS_MAX_LEN = 65535
MIB = 1 << 20                                                  # the smallest chunk_bytes the option takes


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def scoring(init, **more):
    sc = S.make_scoring({"init": [*init, *([0] * (10 - len(init)))], **more})
    return sc, O.Scoring.from_buffer_copy(bytes(sc))


def run(fn, *args, **kw):
    """fn(*args); an error passes through, but never the hand-off time-out."""
    try:
        return fn(*args, **kw)
    except S.SeqAlignError as e:
        assert "timed out" not in str(e), str(e)
        raise


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def related(rng, n, edits=0.05, alphabet=b"ACGT"):
    a = rand_seq(rng, n, alphabet)
    return a, BL.mutate(rng, a, edits, alphabet)


def per_pair(x, n):
    return [x] * n if np.isscalar(x) else list(x)


def same_bytes(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def clamp32(x):
    return max(-2 ** 31, min(2 ** 31 - 1, x))


def check(ctx, sc, osc, pairs, lo, hi, want=None, batch=None):
    """The wide span call on the batch against the oracle's banded hit, against the wide score call and, where they accept the
    batch, the narrow span call and the wide statistics call; returns the wanted [(score cell, five values)]."""
    n = len(pairs)
    lo, hi = per_pair(lo, n), per_pair(hi, n)
    want = want or [BSP.want(osc, a, b, lo[p], hi[p]) for p, (a, b) in enumerate(pairs)]
    batch = batch or W.from_pairs(pairs)
    res = run(ctx.sw_span_banded_wide, batch, sc, lo, hi)
    assert [r.dtype for r in res] == [np.int32] + [np.uint32] * 4 and all(r.shape == (n,) for r in res)
    got = BW.got_spans(res)
    bad = [(p, len(pairs[p][0]), len(pairs[p][1]), lo[p], hi[p], got[p], want[p][1]) for p in range(n) if got[p] != want[p][1]]
    assert not bad, (len(bad), bad[:3])
    score, end_a, end_b = run(ctx.sw_score_banded_wide, batch, sc, lo, hi)
    ends = [(int(score[p]), int(end_a[p]), int(end_b[p])) for p in range(n)]
    assert ends == [(g[0], g[1] + g[3], g[2] + g[4]) for g in got] == [w[0] for w in want]
    if all(BS.width_of(len(a), len(b), lo[p], hi[p]) <= NARROW_MAX for p, (a, b) in enumerate(pairs)):
        assert same_bytes(res, ctx.sw_span_banded(batch, sc, lo, hi))
    if all(max(len(a), len(b)) <= STATS_MAX_LEN for a, b in pairs):
        assert same_bytes(res, run(ctx.sw_stats_banded_wide, batch, sc, lo, hi)[:5])
    return want


def n_hits(want):
    return sum(1 for cell, five in want if five[0] > 0)


# ---------------------------------------------------------------- 1. the definition --
def _protein():
    presets = json.loads((Path(__file__).resolve().parent / "golden" / "presets.json").read_text())
    sc = S.make_scoring({"preset": "BLOSUM62"})
    assert bytes(O.build_scoring(presets["BLOSUM62"]["spec"]))[:8] == bytes(sc)[:8]
    return sc, O.Scoring.from_buffer_copy(bytes(sc)), b"ARNDCQEGHILKMFPSTWYV"


SW_SCORINGS = {
    "plain": lambda: (*scoring(PLAIN), b"ACGT"),
    "no_mismatches": lambda: (*scoring([2, -3, -4, -1, 0, 0, 0, 0, 1]), b"ACGT"),
    "BLOSUM62": _protein,
}


def definition_pairs(rng, n, alphabet):
    """tests/test_gpu_band_wide.py: test_definition_sw's draw: pairs of 0 .. 300 letters, random bounds in +-350."""
    pairs, lo, hi = [], [], []
    for k in range(n):
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
    return pairs, lo, hi


@pytest.mark.parametrize("name", list(SW_SCORINGS))
def test_definition(ctx, name):
    sc, osc, alphabet = SW_SCORINGS[name]()
    pairs, lo, hi = definition_pairs(random.Random(len(name) + 350), 48, alphabet)
    lo[0], hi[0] = 310, 350            # wholly right: empty after clipping for every len_a <= 300
    lo[1], hi[1] = -350, -5            # wholly left
    kinds = {("empty" if BS.clip(len(a), len(b), l, h) is None else "left" if h < 0 else "right" if l > 64 else "mid")
             for (a, b), l, h in zip(pairs, lo, hi)}
    assert kinds == {"empty", "left", "right", "mid"}, kinds
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 16, n_hits(want)


def test_definition_all_flag_combinations(ctx):
    hits = 0
    with ctx.options(band_strip_cols=64):
        for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
            spec = BSP.flag_scoring(idx, flags)
            sc = S.make_scoring(spec)
            osc = O.Scoring.from_buffer_copy(bytes(sc))
            alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
            pairs, lo, hi = definition_pairs(random.Random(7100 + idx), 8, alpha)
            hits += n_hits(check(ctx, sc, osc, pairs, lo, hi))
    assert hits >= 32 * 8 // 3, hits


# ---------------------------------------------------------------- 2. strip geometry --
@pytest.fixture(scope="module")
def geometry(ctx):
    """bandspanwidelib.geometry_cases, the oracle's results and the narrow calls' (computed once)."""
    pairs, lo, hi = BW.geometry_cases()
    sc, osc = scoring(PLAIN)
    assert len(pairs) == len(BW.GEOMETRY_LEN_A) * 5 * 9 * 3
    assert all(BS.width_of(len(a), len(b), l, h) <= NARROW_MAX for (a, b), l, h in zip(pairs, lo, hi))
    assert {max(1, -(-len(a) // 64)) for a, _ in pairs} == {1, 2, 3, 4, 5, 6}
    want = [BSP.want(osc, a, b, l, h) for (a, b), l, h in zip(pairs, lo, hi)]
    assert n_hits(want) >= len(pairs) // 3
    kinds = {BW.band_kind(len(a), len(b), l, h) for (a, b), l, h in zip(pairs, lo, hi)}
    late = sum(BW.late_first_rows(len(a), len(b), l, h, 64) for (a, b), l, h in zip(pairs, lo, hi))
    assert kinds == {"empty", "left", "right", "mid"} and late > 0, (kinds, late)      # empty bands; strips whose first row is late
    batch = W.from_pairs(pairs)
    return dict(n=len(pairs), lo=lo, hi=hi, sc=sc, want=want, batch=batch, narrow=ctx.sw_span_banded(batch, sc, lo, hi),
                score=ctx.sw_score_banded(batch, sc, lo, hi))


@pytest.mark.parametrize("cols", [64, 128, 256, 512, 0])
def test_strip_geometry(ctx, geometry, cols):
    g = geometry
    with ctx.options(band_strip_cols=cols):
        res = run(ctx.sw_span_banded_wide, g["batch"], g["sc"], g["lo"], g["hi"])
        score = run(ctx.sw_score_banded_wide, g["batch"], g["sc"], g["lo"], g["hi"])
        stats = run(ctx.sw_stats_banded_wide, g["batch"], g["sc"], g["lo"], g["hi"])
    got = BW.got_spans(res)
    bad = [(p, int(g["batch"].len_a[p]), int(g["batch"].len_b[p]), g["lo"][p], g["hi"][p], got[p], g["want"][p][1])
           for p in range(g["n"]) if got[p] != g["want"][p][1]]
    assert not bad, (len(bad), bad[:5])
    assert same_bytes(res, g["narrow"]) and same_bytes(score, g["score"]) and same_bytes(res, stats[:5])
    assert np.array_equal(res[0], score[0]) and np.array_equal(res[1] + res[3], score[1]) and np.array_equal(res[2] + res[4], score[2])


# ---------------------------------------------------------------- 3. past 512 and past 1 024 diagonals --
@pytest.fixture(scope="module")
def wide_sw():
    """tests/test_gpu_band_wide.py: wide_sw's two cases of 2 600 letters (1 401 and 1 201 diagonals), and the first pair again
    at 600."""
    sc, osc = scoring(PLAIN)
    rng = random.Random(2600)
    a, b = related(rng, 2600, 0.08)
    b = (rand_seq(rng, 40) + b)[:2600]
    c = rand_seq(rng, 2600)
    d = BL.mutate(rng, c[900:1900], 0.08) + rand_seq(rng, 200)          # lies along diagonals near +900
    cases = [(a, b, -700, 700), (c, d[:1200], 500, 1700), (a, b, -340, 259)]
    return sc, osc, cases, [BSP.want(osc, *case) for case in cases]


@pytest.mark.parametrize("cols", [0, 64])
def test_past_512_and_past_1024(ctx, wide_sw, cols):
    sc, osc, cases, want = wide_sw
    assert [BS.width_of(len(a), len(b), lo, hi) for a, b, lo, hi in cases] == [1401, 1201, 600]
    assert all(w[1][0] > 100 and w[1][3] > 500 and w[1][4] > 500 for w in want), want
    pairs = [(a, b) for a, b, _, _ in cases]
    lo, hi = [c[2] for c in cases], [c[3] for c in cases]
    for p in range(3):                                          # the narrow call refuses each of them
        with pytest.raises(S.SeqAlignError) as e:
            ctx.sw_span_banded(W.from_pairs([pairs[p]]), sc, lo[p], hi[p])
        assert e.value.code == S.E_TOO_LARGE and "pair 0:" in str(e.value)
    with ctx.options(band_strip_cols=cols):
        check(ctx, sc, osc, pairs, lo, hi, want)
        hits = run(ctx.sw_align_banded_wide, W.from_pairs(pairs), sc, lo, hi, 1)
        got = BW.got_spans(run(ctx.sw_span_banded_wide, W.from_pairs(pairs), sc, lo, hi))
    assert all(len(h) == 1 for h in hits) and got == [BSP.fields(h[0]) for h in hits]      # the GPU's own align call's hit fields


# ---------------------------------------------------------------- 4. past 65 535 letters --
def long_pair(case):
    """One sequence of 70 000 letters and a short one of 180, a hit of 120 letters (three of them substituted) between columns /
    rows 69 640 and 69 760 of the long one, a band of 600 diagonals around it.
    "a": len_a = 70 000: 1 094 strips of 64 columns, the band 69 300 .. 69 899 runs off the right side while the hit is swept, the
         last strips' frames overhang len_a, and the best cell is merged across a thousand entries.
    "b": len_b = 70 000, 180 columns in 3 strips, the band -69 900 .. -69 301 at the bottom."""
    rng = random.Random(70 + len(case))
    core = bytes(rng.choice(b"GT") for _ in range(120))
    core2 = bytearray(core)
    for k in (30, 60, 90):
        core2[k] = ord("G") + ord("T") - core2[k]                    # G <-> T: a mismatch inside the hit
    long_ = bytearray(rng.choice(b"AC") for _ in range(70000))
    short = bytearray(rng.choice(b"KM") for _ in range(180))
    long_[69640:69760] = core
    short[40:160] = core2
    if case == "a":
        return (bytes(long_), bytes(short)), 69300, 69899
    return (bytes(short), bytes(long_)), -69900, -69301


@pytest.mark.parametrize("case", ["a", "b"])
def test_past_65535_letters(ctx, case):
    """The new ground: coordinates above 65 535 come back exactly, where sw_stats_banded_wide refuses the batch."""
    sc, osc = scoring(PLAIN)
    (a, b), lo, hi = long_pair(case)
    assert max(len(a), len(b)) == 70000 and min(len(a), len(b)) == 180 and BS.width_of(len(a), len(b), lo, hi) == 600
    assert max(1, -(-len(a) // 64)) == (1094 if case == "a" else 3)
    batch = W.from_pairs([(a, b)])
    for fn in (ctx.sw_stats_banded_wide, ctx.sw_span_banded, ctx.sw_stats_banded):
        with pytest.raises(S.SeqAlignError) as e:
            fn(batch, sc, lo, hi)
        assert e.value.code == S.E_TOO_LARGE, str(e.value)
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, [(a, b)], lo, hi, batch=batch)
        if case == "a":
            assert ctx.last_call()["band_score"][1] >= 10            # (the score call's busy strips: the band's columns alone)
    assert want[0][1] == ((225, 69640, 40, 120, 120) if case == "a" else (225, 40, 69640, 120, 120)), want
    for cols in (0, 512):                                           # the widest strips and the default: the same five
        with ctx.options(band_strip_cols=cols):
            assert BW.got_spans(run(ctx.sw_span_banded_wide, batch, sc, lo, hi)) == [want[0][1]]


# ---------------------------------------------------------------- 5. ties --
def test_equal_best_cells_in_several_strips(ctx):
    """unit x 6 against unit and the reverse: the best cell occurs once per repeat, in different strips; the lowest column wins."""
    sc, osc = scoring(PLAIN)
    unit = rand_seq(random.Random(6), 40)
    with ctx.options(band_strip_cols=64):
        for a, b in ((unit * 6, unit), (unit, unit * 6)):
            la, lb = len(a), len(b)
            for lo, hi in ((-lb, la), (-FULL, FULL - 1), (45, la), (-lb, 100), (-130, -50), (70, 170), (-lb, -15)):
                if lo > hi:                                # (45, la) on the 40-letter seq_a
                    continue
                want = check(ctx, sc, osc, [(a, b)], lo, hi)
                if lo <= -lb and hi >= la:
                    assert want[0][1] == (80, 0, 0, 40, 40), want


@pytest.mark.parametrize("name", list(SP.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_across_seams(ctx, name):
    """bandspanlib.tie_batch (len_a near 200 and 400: 4 and 7 strips of 64 columns) with bandspanlib.TIE_BANDS, which put seams
    through the hits.  Every batch and band holds a pair whose wanted span changes under the reversed priority (the narrow call's
    floor, test_sw_span_banded_argument_cpu.py), found here on the oracle alone."""
    sc, osc = scoring(SP.TIE_SCORINGS[name])
    crossing = 0
    with ctx.options(band_strip_cols=64):
        for width in BSP.TIE_WIDTHS:
            pairs = BSP.tie_batch(name, width)
            for lo, hi in BSP.TIE_BANDS:
                want = check(ctx, sc, osc, pairs, lo, hi)
                assert n_hits(want) >= 30, n_hits(want)
                crossing += sum(BW.crosses_seam(five, 64) for cell, five in want)
                assert any(BSP.reversed_differs(osc, a, b, lo, hi) for a, b in pairs), (name, width, lo, hi)
    assert crossing >= 20, crossing


# ---------------------------------------------------------------- 6. a gap that pays --
def test_a_gap_that_pays_starts_hits_outside_the_band(ctx):
    """tests/test_gpu_sw_span_banded.py's scoring and shapes (reads of 150 in windows of 200, gap_extend = +1), the reads in
    seq_a's columns 40 .. 189 of 3 strips so that the band's left edge, and with it the outside start, lies in a strip left of the
    seam the hit crosses."""
    rng = random.Random(404)
    sc, osc = scoring([2, -3, -2, 1])
    pairs, lo, hi = [], [], []
    for _ in range(40):
        read, window, offset = BS.read_in_window(rng, 150, 200, 0.08)
        pairs.append((rand_seq(rng, 40) + read, window))
        lo.append(40 - offset - 4)
        hi.append(40 - offset + 4)
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, pairs, lo, hi)
    outside = [p for p, ((a, b), (cell, five)) in enumerate(zip(pairs, want)) if BSP.starts_outside(five, len(a), len(b), lo[p], hi[p])]
    left = [p for p in outside if BW.outside_left_of_seam(want[p][1], len(pairs[p][0]), len(pairs[p][1]), lo[p], hi[p], 64)]
    print("starts outside the band:", len(outside), "of them left of a seam:", len(left), "of", n_hits(want))
    assert len(outside) >= 10 and len(left) >= 5, (len(outside), len(left))


# ---------------------------------------------------------------- 7. mixed batch and chunks --
def model_bytes(la, lb, lo, hi, cols=64):
    """The contract's device bytes of one pair (an empty band is handed to the kernel as one diagonal)."""
    strips = max(1, -(-la // cols))
    return la + lb + 88 + strips * (32 * max(1, BS.width_of(la, lb, lo, hi)) + 36) + 20


def busy_strips(la, lb, lo, hi, cols):
    """The (pair, strip) waves that sweep a row: the strips that hold a column with an inner band cell."""
    band = BS.clip(la, lb, lo, hi)
    if band is None or la == 0 or lb == 0:
        return 0
    c_lo, c_hi = max(1, 1 + band[0]), min(la, lb + band[1])
    return 0 if c_lo > c_hi else (c_hi - 1) // cols - (c_lo - 1) // cols + 1


MIXED = [(0, 30, -5, 5), (40, 44, 0, 0), (64, 60, -10, 10), (100, 100, 0, 0), (128, 90, -30, 30), (300, 310, -16, 16),
         (320, 300, -200, 200), (1, 1, 0, 0), (300, 0, 0, 0), (50, 50, -FULL, FULL - 1), (65, 64, -1, 1), (127, 127, -63, 63),
         (290, 257, -2, 2), (30, 0, 0, 0), (0, 0, 0, 0), (310, 310, 20, 53), (90, 128, -70, -7), (257, 320, -100, 100),
         (250, 192, 300, 400), (0, 1, 0, 0), (192, 192, -64, 64), (300, 300, -299, -250), (280, 40, 100, 260)] * 3
MIXED_REPEATS = 5


def test_mixed_batch_and_chunks(ctx):
    """69 ragged pairs of 1 .. 5 strips, empty sequences and empty bands among them, checked against the oracle; the batch five
    times over is several MB by the contract's formula, which chunk_bytes = 1 MiB cuts into chunks by the greedy rule."""
    sc, osc = scoring(PLAIN)
    rng = random.Random(606)
    base = []
    for la, lb, lo, hi in MIXED:
        a = rand_seq(rng, la)
        base.append((a, (BL.mutate(rng, a, 0.05) + rand_seq(rng, lb))[:lb]))
    lo, hi = [clamp32(m[2]) for m in MIXED], [clamp32(m[3]) for m in MIXED]
    assert {max(1, -(-m[0] // 64)) for m in MIXED} == {1, 2, 3, 4, 5}
    assert {BW.band_kind(m[0], m[1], m[2], m[3]) for m in MIXED} == {"empty", "left", "right", "mid"}
    pairs = base * MIXED_REPEATS
    batch, los, his = W.from_pairs(pairs), lo * MIXED_REPEATS, hi * MIXED_REPEATS
    chunks, used = 1, 0
    for la, lb, l, h in MIXED * MIXED_REPEATS:                 # the greedy cut of the contract
        x = model_bytes(la, lb, l, h)
        if used and used + x > MIB:
            chunks, used = chunks + 1, 0
        used += x
    assert chunks >= 3
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, base, lo, hi)
        assert n_hits(want) >= 30
        one = run(ctx.sw_span_banded_wide, batch, sc, los, his)
        assert ctx.last_call()["band_score"][0] == 1 and BW.got_spans(one) == [five for cell, five in want] * MIXED_REPEATS
        with ctx.options(chunk_bytes=MIB):
            cut = run(ctx.sw_span_banded_wide, batch, sc, los, his)
            assert ctx.last_call()["band_score"][0] == chunks, (ctx.last_call(), chunks)
        assert same_bytes(cut, one)


def test_a_pair_that_does_not_fit_the_budget(ctx):
    """320 x 7 000 with the whole matrix as its band: 5 strips of 64 columns, 7 321 diagonals.  At the formula's budget the call
    runs (and is the unbanded call's result); one byte under it is E_NOMEM with the bytes named."""
    sc, _ = scoring(PLAIN)
    rng = random.Random(7000)
    a = rand_seq(rng, 320)
    b = (rand_seq(rng, 3000) + BL.mutate(rng, a, 0.05) + rand_seq(rng, 7000))[:7000]
    small = (rand_seq(rng, 70), rand_seq(rng, 66))
    batch, lo, hi = W.from_pairs([small, (a, b), small]), [-3, -7000, -3], [3, 320, 3]
    need = model_bytes(320, 7000, -7000, 320)
    assert need == 320 + 7000 + 88 + 5 * (32 * 7321 + 36) + 20 and need - 1 >= MIB
    with ctx.options(band_strip_cols=64):
        with ctx.options(chunk_bytes=need):
            got = run(ctx.sw_span_banded_wide, batch, sc, lo, hi)
            assert ctx.last_call()["band_score"][0] == 3                # each pair a chunk of its own
        full = ctx.sw_span(W.from_pairs([(a, b)]), sc)
        assert [int(x[1]) for x in got] == [int(x[0]) for x in full] and int(got[3][1]) > 250
        with ctx.options(chunk_bytes=need - 1):
            with pytest.raises(S.SeqAlignError) as e:
                run(ctx.sw_span_banded_wide, batch, sc, lo, hi)
        assert e.value.code == S.E_NOMEM and "pair 1:" in str(e.value) and f" {need} bytes" in str(e.value), str(e.value)


# ---------------------------------------------------------------- 8. errors and accounting --
def test_errors_and_their_order_on_a_live_context(ctx):
    sc, _ = scoring(PLAIN)
    rng = random.Random(8)
    short, long_ = (rand_seq(rng, 50), rand_seq(rng, 60)), (rand_seq(rng, STATS_MAX_LEN + 1, b"AC"), rand_seq(rng, 20, b"GT"))
    for pairs, lo, hi, text in (
            ([short, short], [-3, 4], [3, 3], "pair 1: diag_lo"),
            ([long_, short, short], [-3, -3, 9], [3, 3, 8], "pair 2: diag_lo"),
            ([short, short, short], [5, -3, 9], [3, 3, 8], "pair 0: diag_lo")):      # the lowest pair first
        for fn in (ctx.sw_span_banded_wide, ctx.sw_span_banded):
            with pytest.raises(S.SeqAlignError) as e:
                run(fn, W.from_pairs(pairs), sc, lo, hi)
            assert e.value.code == S.E_ARG and text in str(e.value), (str(e.value), text)
    with pytest.raises(S.SeqAlignError) as e:                   # the narrow call reports the width, the pair named
        ctx.sw_span_banded(W.from_pairs([short, long_]), sc, -700, 700)
    assert e.value.code == S.E_TOO_LARGE and "pair 1:" in str(e.value)
    with ctx.options(band_strip_cols=64):
        res = run(ctx.sw_span_banded_wide, W.from_pairs([short, long_]), sc, -700, 700)      # 65 536 letters are taken
    assert int(res[0][1]) == 0 and ctx.last_call() == {"band_score": (1, 1 + 12)}, ctx.last_call()   # columns 1 .. 720: 12 strips


def test_accounting(ctx):
    sc, _ = scoring(PLAIN)
    rng = random.Random(11)
    pairs = [related(rng, n) for n in (0, 30, 64, 65, 200, 640, 700)] + [(rand_seq(rng, 100), b""), (b"", rand_seq(rng, 9))]
    batch = W.from_pairs(pairs)
    for cols in (64, 256, 512):
        for lo, hi in ((-10, 10), (100, 330), (-FULL, -70), (650, 660)):
            lo, hi = clamp32(lo), clamp32(hi)
            busy = sum(busy_strips(len(a), len(b), lo, hi, cols) for a, b in pairs)
            with ctx.options(band_strip_cols=cols):
                run(ctx.sw_span_banded_wide, batch, sc, lo, hi)
            assert ctx.last_call() == {"band_score": (1, busy)}, (cols, lo, hi, ctx.last_call(), busy)


def test_unknown_pair_inside_and_outside_the_band(ctx):
    """X (in seq_a) against Y (in seq_b) has no score; every other pair of letters has one."""
    sc = S.make_scoring({"preset": "DNA_hybridization",
                         "mutations": [["x", c, -1] for c in "acgt"] + [[c, "y", -1] for c in "acgt"]})
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    a = b"ACGGTCATTG" * 60
    b = a[:290] + b"T" + a[290:]
    with_x = a[:300] + b"X" + a[301:]              # column 301: the fifth strip of 64
    near = b[:302] + b"Y" + b[303:]                # row 303 against column 301: diagonal -2
    far = b[:20] + b"Y" + b[21:]                   # row 21 against column 301: diagonal 280
    good = (a, b)
    assert BS.fill_unknown(osc, with_x, near, (-8, 8))[3] == [(301, 303)]
    assert BS.fill_unknown(osc, with_x, far, (-8, 8))[3] == []
    inside = W.from_pairs([good, good, (with_x, far), (with_x, near), good, (with_x, near)])
    with ctx.options(band_strip_cols=64):
        with pytest.raises(S.SeqAlignError) as want:
            ctx.sw_span_banded(inside, sc, -8, 8)
        with pytest.raises(S.SeqAlignError) as got:
            run(ctx.sw_span_banded_wide, inside, sc, -8, 8)
        assert got.value.code == S.E_UNKNOWN_PAIR and "pair 3:" in str(got.value), str(got.value)
        assert str(got.value).split("] ")[-1] == str(want.value).split("] ")[-1]
        res = check(ctx, sc, osc, [good, (with_x, far), good], -8, 8)
        assert n_hits(res) == 3 and res[0] == res[2]
        # past the narrow cap the far pair meets X against Y inside the band
        with pytest.raises(S.SeqAlignError) as got:
            run(ctx.sw_span_banded_wide, W.from_pairs([good, (with_x, far)]), sc, -300, 300)
        assert got.value.code == S.E_UNKNOWN_PAIR and "pair 1:" in str(got.value), str(got.value)


# ---------------------------------------------------------------- 9. the int32 domain and the scorings off the fast path --
def test_large_magnitudes_inside_and_outside_the_admitted_domain(ctx):
    """maglib's `steep` scoring on its 96 x 96 pairs under a band of 17 diagonals around each pair's corner diagonal: at the
    largest scale the documented rule admits (maglib.admitted, call "band") the five outputs equal the oracle's and the narrow
    call's; one scale further both calls are SEQALIGN_E_DOMAIN and nothing is launched."""
    base = G.BASES["steep"]
    pairs = [G.pair("sq", kind) for kind in G.kinds_of("sq")]
    la, lb = max(len(a) for a, _ in pairs), max(len(b) for _, b in pairs)
    band_lo = [len(a) - len(b) - 8 for a, b in pairs]
    band_hi = [len(a) - len(b) + 8 for a, b in pairs]
    lo, hi = 1, 1 << 31
    while hi - lo > 1:                       # the rule is monotone in the scale
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if G.admitted(G.scaled(base, mid), la, lb, "band") else (lo, mid)
    inside, outside = G.scaled(base, lo), G.scaled(base, hi)
    assert G.admitted(inside, la, lb, "band") and not G.admitted(outside, la, lb, "band")
    sc = S.make_scoring(inside)
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, G.oracle_scoring(inside), pairs, band_lo, band_hi)
        assert max(w[1][0] for w in want) > 1 << 30, [w[1][0] for w in want]
        run(ctx.sw_span_banded_wide, W.from_pairs(pairs[:1]), scoring(PLAIN)[0], -8, 8)
        for fn in (ctx.sw_span_banded_wide, ctx.sw_span_banded):
            with pytest.raises(S.SeqAlignError) as err:
                run(fn, W.from_pairs(pairs), S.make_scoring(outside), band_lo, band_hi)
            assert err.value.code == S.E_DOMAIN and str(G.INT32_MAX) in str(err.value), str(err.value)
            assert not ctx.last_call(), ctx.last_call()


OFF_FAST = {"gap_open+": [5, -4, 3, -4], "gap_extend+": [3, -2, -5, 1], "free_ends": [1, -2, -4, -1, 1, 1]}


@pytest.mark.parametrize("name", list(OFF_FAST))
def test_off_the_fast_path(ctx, name):
    sc, osc = scoring(OFF_FAST[name])
    rng = random.Random(65)
    pairs, lo, hi = [], [], []
    for lb in (65, 129, 193):                      # one past a multiple of 64; len_a = 65: the last column alone in its strip
        a = rand_seq(rng, 65)
        for w in (0, 3, 40, 64, 200):
            pairs.append((a, (BL.mutate(rng, a, 0.1) + rand_seq(rng, lb))[:lb]))
            lo.append(-w - 2)
            hi.append(w)
    a = rand_seq(rng, 260)
    for w in (5, 70, 300):
        pairs.append((a, BL.mutate(rng, a, 0.1)))
        lo.append(-w)
        hi.append(w + 1)
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 12
