"""GPU tier: wide banded NW statistics -- seqalign_nw_stats_banded_wide (sa_band_nw_stats_strips.hip, sa_batch_band.hip).

The contract is seqalign_nw_stats_banded's at any width.  Results are checked bit for bit against the oracle (bandnwstatlib.want:
the banded end value and the counted columns of its walk over the banded matrices, or SEQALIGN_E_TRACEBACK naming the lowest pair
that has no alignment inside its band), the score against ctx.nw_score_banded_wide, and all three arrays against
ctx.nw_stats_banded byte for byte wherever the narrow call accepts the batch.  Unless stated the strips are forced to 64 columns
(option band_strip_cols), so that small pairs have several strips.  No call may return the hand-off time-out."""
import json
import random
from pathlib import Path

import numpy as np
import pytest

import bandlib as BL
import bandnwstatlib as BN
import bandnwstatwidelib as BW
import denselib as D
import orclib as O
import seqalign_amd as S
import statlib as ST
from seqalign_amd import workloads as W

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


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def related(rng, n, edits=0.05, alphabet=b"ACGT"):
    a = rand_seq(rng, n, alphabet)
    return a, BL.mutate(rng, a, edits, alphabet)


def same_bytes(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def check(ctx, sc, osc, triples, want=None):
    """The wide statistics call on [(a, b, w)] against `want` (bandnwstatlib.want per triple; None: no alignment inside the
    band).  A batch with such pairs must raise E_TRACEBACK naming the lowest, and is checked without them.  Returns want."""
    want = want or [BN.want(osc, a, b, w) for a, b, w in triples]
    none = [p for p, x in enumerate(want) if x is None]
    if none:
        with pytest.raises(S.SeqAlignError) as e:
            run(ctx.nw_stats_banded_wide, W.from_pairs([(a, b) for a, b, _ in triples]), sc, [w for _, _, w in triples])
        assert e.value.code == S.E_TRACEBACK and f"pair {none[0]}:" in str(e.value), (str(e.value), none)
    kept = [p for p, x in enumerate(want) if x is not None]
    if not kept:
        return want
    batch = W.from_pairs([triples[p][:2] for p in kept])
    bands = [triples[p][2] for p in kept]
    res = run(ctx.nw_stats_banded_wide, batch, sc, bands)
    assert [r.dtype for r in res] == [np.int32, np.uint32, np.uint32] and all(r.shape == (len(kept),) for r in res)
    got = ST.got_stats(res)
    bad = [(p, len(triples[p][0]), len(triples[p][1]), triples[p][2], got[k], want[p]) for k, p in enumerate(kept) if got[k] != want[p]]
    assert not bad, (len(bad), bad[:3])
    assert res[0].tobytes() == run(ctx.nw_score_banded_wide, batch, sc, bands).tobytes()
    if all(BL.width_of(len(triples[p][0]), len(triples[p][1]), triples[p][2]) <= NARROW_MAX for p in kept):
        assert same_bytes(res, ctx.nw_stats_banded(batch, sc, bands))
    return want


# ---------------------------------------------------------------- 1. the definition --
def test_definition_all_flag_combinations(ctx):
    """bandnwstatwidelib.definition_cases; which of its pairs have no alignment inside their band is held against the end
    value on the oracle in test_magnitude_argument_cpu.py."""
    n_none = 0
    cases = BW.definition_cases()
    assert len(cases) == 32
    with ctx.options(band_strip_cols=64):
        for init, triples in cases:
            sc, osc = scoring(init)
            want = check(ctx, sc, osc, triples)
            n_none += sum(x is None for x in want)
    assert n_none > 0


# ---------------------------------------------------------------- 2. strip geometry --
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
    """The cases, the oracle's results and the narrow call's (computed once)."""
    pairs, bands = geometry_cases()
    sc, osc = scoring(PLAIN)
    assert len(pairs) == 405 and all(BL.width_of(len(a), len(b), w) <= NARROW_MAX for (a, b), w in zip(pairs, bands))
    want = [BN.want(osc, a, b, w) for (a, b), w in zip(pairs, bands)]
    assert None not in want
    batch = W.from_pairs(pairs)
    return dict(bands=bands, sc=sc, want=want, batch=batch, narrow=ctx.nw_stats_banded(batch, sc, bands))


@pytest.mark.parametrize("cols", [64, 128, 256, 512, 0])
def test_strip_geometry(ctx, geometry, cols):
    g = geometry
    with ctx.options(band_strip_cols=cols):
        res = run(ctx.nw_stats_banded_wide, g["batch"], g["sc"], g["bands"])
    got = ST.got_stats(res)
    bad = [(p, int(g["batch"].len_a[p]), int(g["batch"].len_b[p]), g["bands"][p], got[p], g["want"][p]) for p in range(405) if got[p] != g["want"][p]]
    assert not bad, (len(bad), bad[:5])
    assert same_bytes(res, g["narrow"])


# ---------------------------------------------------------------- 3. past the narrow caps --
@pytest.fixture(scope="module")
def past_caps():
    rng = random.Random(513)
    sc, osc = scoring(PLAIN)
    cases = []
    for w, tail in ((300, 0), (600, 0), (300, -40), (600, 35)):
        a, b = related(rng, 1300, 0.06)
        cases.append((a + rand_seq(rng, tail), b, w) if tail > 0 else (a, b + rand_seq(rng, -tail), w))
    widths = [BL.width_of(len(a), len(b), w) for a, b, w in cases]
    assert all(600 < x <= 1024 for x in widths[0::2]) and all(x > 1200 for x in widths[1::2]), widths
    a, b = related(rng, 700, 0.1)
    whole = (a, (b + rand_seq(rng, 100))[:650])
    assert BL.width_of(700, 650, FULL) == 1351
    return sc, osc, cases, whole


@pytest.mark.parametrize("cols", [64, 0])
def test_past_the_narrow_caps(ctx, past_caps, cols):
    sc, osc, cases, whole = past_caps
    batch, bands = W.from_pairs([c[:2] for c in cases]), [c[2] for c in cases]
    with pytest.raises(S.SeqAlignError) as e:
        ctx.nw_stats_banded(batch, sc, bands)                  # the narrow call refuses these
    assert e.value.code == S.E_TOO_LARGE
    with ctx.options(band_strip_cols=cols):
        res = run(ctx.nw_stats_banded_wide, batch, sc, bands)
        aligned = run(ctx.nw_align_banded_wide, batch, sc, bands)
        assert res[0].tobytes() == run(ctx.nw_score_banded_wide, batch, sc, bands).tobytes()
        full = run(ctx.nw_stats_banded_wide, W.from_pairs([whole]), sc, FULL)
    got = ST.got_stats(res)
    assert got == [(score,) + ST.count_columns(osc, ra, rb) for score, ra, rb in aligned]
    assert all(g[1] > 1000 and g[2] > 10 for g in got), got
    assert same_bytes(full, ctx.nw_stats(W.from_pairs([whole]), sc))


# ---------------------------------------------------------------- 4. ties and gaps across seams --
TIE_CASES = ((64, 20), (200, 150), (700, 400))      # (statlib.tie_pairs' width, w): 1, 4 and 11 strips of 64 columns


@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_across_seams(ctx, name):
    sc, osc = scoring(ST.TIE_SCORINGS[name])
    sensitive = 0
    with ctx.options(band_strip_cols=64):
        for width, w in TIE_CASES:
            pairs = BN.tie_batch(name, width)
            want = check(ctx, sc, osc, [(a, b, w) for a, b in pairs])
            assert None not in want
            sensitive += sum(BN.counts_reversed_differ(osc, a, b, w) for a, b in pairs)
    assert sensitive >= 10, sensitive


def test_alternation_across_seams(ctx):
    """denselib's alternation: an insertion run against a deletion run on every period, 21 strips of 64 columns."""
    sc, osc = scoring([2, -9, 0, -1])
    triples = [(*D.alternation(1300, 1300, k), w) for k, w in ((0, 3), (1, 40), (2, 600))]
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, triples)
    assert None not in want


# ---------------------------------------------------------------- 5. counts past 65 535 --
def test_counts_past_65535(ctx):
    rng = random.Random(70001)
    n, k = 70000, 9
    sc, _ = scoring([1, -1, -10, -1])
    a = bytearray(rand_seq(rng, n))
    b = bytearray(a)
    for at in rng.sample(range(n), k):
        b[at] = b"ACGT"[(b"ACGT".index(b[at]) + 1 + rng.randrange(3)) % 4]
    batch = W.from_pairs([(bytes(a), bytes(b))])
    with ctx.options(band_strip_cols=512):
        res = run(ctx.nw_stats_banded_wide, batch, sc, 3)
    assert same_bytes(res, ctx.nw_stats_banded(batch, sc, 3))
    assert int(res[1][0]) > 65535 and ST.got_stats(res) == [(n - 2 * k, n - k, k)], ST.got_stats(res)


# ---------------------------------------------------------------- 6. mixed batch and chunks --
def model_bytes(la, lb, w, cols=64):
    """The contract's device bytes of one pair."""
    strips = max(1, -(-la // cols))
    return la + lb + 72 + strips * (32 * BL.width_of(la, lb, w) + 20) + 20


MIB = 1 << 20                                                  # the smallest chunk_bytes the option takes
MIXED = [(0, 30, 5), (40, 44, 0), (64, 60, 10), (100, 100, 0), (128, 90, 30), (300, 310, 16), (320, 300, 200), (1, 1, 0),
         (300, 0, 0), (50, 50, FULL), (65, 64, 1), (127, 127, 63), (290, 257, 2), (30, 0, 0), (0, 0, 0), (310, 310, 33),
         (90, 128, 7), (257, 320, 100), (250, 192, 64), (0, 1, 0), (192, 192, 64)] * 3
MIXED_REPEATS = 5


def test_mixed_batch_and_chunks(ctx):
    """63 ragged pairs of 1 .. 5 strips, empty sequences among them, checked against the oracle; the batch five times over is
    3.8 MB by the contract's formula, which chunk_bytes = 1 MiB cuts into several chunks."""
    sc, osc = scoring(PLAIN)
    rng = random.Random(606)
    base = []
    for la, lb, w in MIXED:
        a = rand_seq(rng, la)
        base.append((a, (BL.mutate(rng, a, 0.05) + rand_seq(rng, lb))[:lb], w))
    assert {max(1, -(-la // 64)) for la, _, _ in MIXED} == {1, 2, 3, 4, 5}
    triples = base * MIXED_REPEATS
    batch, bands = W.from_pairs([t[:2] for t in triples]), [t[2] for t in triples]
    chunks, used = 1, 0
    for la, lb, w in MIXED * MIXED_REPEATS:                    # the greedy cut of the contract
        x = model_bytes(la, lb, w)
        if used and used + x > MIB:
            chunks, used = chunks + 1, 0
        used += x
    assert chunks >= 4
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, base)
        assert None not in want
        one = run(ctx.nw_stats_banded_wide, batch, sc, bands)
        assert ctx.last_call()["band_score"][0] == 1 and ST.got_stats(one) == want * MIXED_REPEATS
        with ctx.options(chunk_bytes=MIB):
            cut = run(ctx.nw_stats_banded_wide, batch, sc, bands)
            assert ctx.last_call()["band_score"][0] == chunks, (ctx.last_call(), chunks)
        assert same_bytes(cut, one)


def test_a_pair_that_does_not_fit_the_budget(ctx):
    """320 x 7 000 with the whole matrix as its band: 5 strips of 64 columns, 7 321 diagonals, 1 178 872 bytes by the contract's
    formula.  At that budget the call runs (and is the unbanded call's result); one byte under it is E_NOMEM with the bytes
    named."""
    sc, _ = scoring(PLAIN)
    rng = random.Random(7000)
    a = rand_seq(rng, 320)
    b = rand_seq(rng, 3000) + BL.mutate(rng, a, 0.05) + rand_seq(rng, 7000)
    small = (rand_seq(rng, 70), rand_seq(rng, 66))
    batch, bands = W.from_pairs([small, (a, b[:7000]), small]), [3, FULL, 3]
    need = model_bytes(320, 7000, FULL)
    assert need == 320 + 7000 + 72 + 5 * (32 * 7321 + 20) + 20 and need - 1 >= MIB
    with ctx.options(band_strip_cols=64):
        with ctx.options(chunk_bytes=need):
            got = run(ctx.nw_stats_banded_wide, batch, sc, bands)
            assert ctx.last_call()["band_score"][0] == 3                # each pair a chunk of its own
        full = ctx.nw_stats(W.from_pairs([(a, b[:7000])]), sc)
        assert [int(x[1]) for x in got] == [int(x[0]) for x in full] and int(got[1][1]) > 250
        with ctx.options(chunk_bytes=need - 1):
            with pytest.raises(S.SeqAlignError) as e:
                run(ctx.nw_stats_banded_wide, batch, sc, bands)
        assert e.value.code == S.E_NOMEM and "pair 1:" in str(e.value) and f" {need} bytes" in str(e.value), str(e.value)


# ---------------------------------------------------------------- 7. errors and accounting --
def test_unknown_pair_no_walk_and_their_order(ctx):
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
    assert BL.fill_unknown(osc, with_x, near, BL.band_of(600, 601, 8))[3] == [(301, 303)]
    assert BL.fill_unknown(osc, with_x, far, BL.band_of(600, 601, 8))[3] == []
    inside = W.from_pairs([good, good, (with_x, far), (with_x, near), good, (with_x, near)])
    with ctx.options(band_strip_cols=64):
        with pytest.raises(S.SeqAlignError) as want:
            ctx.nw_stats_banded(inside, sc, 8)
        with pytest.raises(S.SeqAlignError) as got:
            run(ctx.nw_stats_banded_wide, inside, sc, 8)
        assert got.value.code == S.E_UNKNOWN_PAIR and "pair 3:" in str(got.value), str(got.value)
        assert str(got.value).split("] ")[-1] == str(want.value).split("] ")[-1]
        res = check(ctx, sc, osc, [(*good, 8), (with_x, far, 8), (*good, 8)])
        assert None not in res and res[0] == res[2]

        # with a pair that has no alignment inside its band: the lower pair's code, as in the narrow call
        strict = S.make_scoring({"preset": "DNA_hybridization",
                                 "flags": {"no_mismatches": True, "no_gaps_in_a": True, "no_gaps_in_b": True}})
        ostrict = O.Scoring.from_buffer_copy(bytes(strict))
        bandless = BN.bandless_pair(200, 160)      # a substitution in strip 2
        c = bandless[0]
        unknown = (c[:150] + b"Z" + c[151:], c[:150] + b"Z" + c[151:])
        same = (c, c)
        assert BN.want(ostrict, *same, 8)[1:] == (200, 0) and BN.want(ostrict, *bandless, 8) is None
        assert BL.fill_unknown(ostrict, *unknown, BL.band_of(200, 200, 8))[3] == [(151, 151)]
        for pairs, code, pair in (([same, bandless, unknown], S.E_TRACEBACK, 1), ([same, unknown, bandless], S.E_UNKNOWN_PAIR, 1),
                                  ([unknown], S.E_UNKNOWN_PAIR, 0), ([same, same, bandless], S.E_TRACEBACK, 2)):
            with pytest.raises(S.SeqAlignError) as want:
                ctx.nw_stats_banded(W.from_pairs(pairs), strict, 8)
            with pytest.raises(S.SeqAlignError) as got:
                run(ctx.nw_stats_banded_wide, W.from_pairs(pairs), strict, 8)
            assert got.value.code == code == want.value.code and f"pair {pair}:" in str(got.value), (str(got.value), code, pair)
            assert str(got.value).split("] ")[-1] == str(want.value).split("] ")[-1]


def test_accounting(ctx):
    sc, _ = scoring(PLAIN)
    rng = random.Random(11)
    pairs = [related(rng, n) for n in (0, 30, 64, 65, 200, 640, 700)] + [(rand_seq(rng, 100), b""), (b"", rand_seq(rng, 9))]
    batch = W.from_pairs(pairs)
    for cols in (64, 256):
        busy = sum(-(-len(a) // cols) for a, b in pairs if len(b))      # every column of a pair with rows has an inner band cell
        with ctx.options(band_strip_cols=cols):
            run(ctx.nw_stats_banded_wide, batch, sc, 10)
        assert ctx.last_call() == {"band_score": (1, busy)}, (cols, ctx.last_call(), busy)


# ---------------------------------------------------------------- 8. off the fast path --
def _protein():
    presets = json.loads((Path(__file__).resolve().parent / "golden" / "presets.json").read_text())
    sc = S.make_scoring({"preset": "BLOSUM62"})
    assert bytes(O.build_scoring(presets["BLOSUM62"]["spec"]))[:8] == bytes(sc)[:8]
    return sc, O.Scoring.from_buffer_copy(bytes(sc))


OFF_FAST = {"gap_open+": [5, -4, 3, -4], "gap_extend+": [3, -2, -5, 1], "free_ends": [1, -2, -4, -1, 1, 1], "BLOSUM62": None}


@pytest.mark.parametrize("name", list(OFF_FAST))
def test_off_the_fast_path(ctx, name):
    (sc, osc), alpha = (_protein(), b"ARNDCQEGHILKMFPSTWYV") if OFF_FAST[name] is None else (scoring(OFF_FAST[name]), b"ACGT")
    rng = random.Random(65)
    triples = []
    for lb in (65, 129, 193):                      # one past a multiple of 64; len_a = 65: the last column alone in its strip
        a = rand_seq(rng, 65, alpha)
        for w in (0, 3, 40, 64, 200):
            triples.append((a, (BL.mutate(rng, a, 0.1, alpha) + rand_seq(rng, lb, alpha))[:lb], w))
    a = rand_seq(rng, 260, alpha)
    triples += [(a, BL.mutate(rng, a, 0.1, alpha), w) for w in (5, 70, 300)]
    with ctx.options(band_strip_cols=64):
        want = check(ctx, sc, osc, triples)
    assert None not in want
