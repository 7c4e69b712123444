"""GPU tier: banded NW -- seqalign_nw_score_banded / seqalign_nw_align_banded (sa_band.hip, sa_batch_band.hip).

The definition (include/seqalign_hip.h) is checked against its Python restatement walked by the oracle (bandlib.expected);
the kernels' frame classes, both phases of the moving frame and the band edges against seqalign_nw_batch through the
in-band property: when nw_batch's own alignment of a pair lies inside a band, the banded result is nw_batch's byte for byte."""
import itertools
import json
import random
from pathlib import Path

import numpy as np
import pytest

import bandlib as BL
import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
FULL = 2 ** 31                                   # a band that covers every matrix
LADDER = [64, 128, 192, 256, 320, 384, 512, 768, 1024]   # widths at which the columns per lane step up
EDGE_WIDTHS = sorted({63, 1023} | set(LADDER) | {w + 1 for w in LADDER if w < 1024})
PLAIN = [1, -2, -4, -1]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def oracle_scoring_of(sc):
    return O.Scoring.from_buffer_copy(bytes(sc))


def rescore(ra: bytes, rb: bytes, match: int, mismatch: int, gap_open: int, gap_extend: int) -> int:
    """Affine score of two gapped strings (plain scoring, no flags): a gap of length L costs gap_open + L * gap_extend."""
    x, y = np.frombuffer(ra, np.uint8), np.frombuffer(rb, np.uint8)
    ga, gb = x == ord("-"), y == ord("-")
    both = ~ga & ~gb
    s = int(np.where(x[both] == y[both], match, mismatch).sum())
    for g in (ga, gb):
        starts = int((g & ~np.concatenate(([False], g[:-1]))).sum())
        s += gap_open * starts + gap_extend * int(g.sum())
    return s


def both_calls(ctx, batch, sc, band):
    """The align call's result, after checking that the score call agrees with it."""
    got = ctx.nw_align_banded(batch, sc, band)
    score = ctx.nw_score_banded(batch, sc, band)
    assert [g[0] for g in got] == [int(s) for s in score]
    return got


def related_pairs(rng, lengths, alphabet=b"ACGT", tails=()):
    """Pairs of a random sequence and an edited copy (2-10 % edits in equal thirds); tails[k] > 0 appends that many random
    letters to seq_a of pair k, < 0 to seq_b."""
    pairs = []
    for k, n in enumerate(lengths):
        a = bytes(rng.choice(alphabet) for _ in range(n))
        b = BL.mutate(rng, a, rng.uniform(0.02, 0.10), alphabet)
        t = tails[k] if k < len(tails) else 0
        extra = bytes(rng.choice(alphabet) for _ in range(abs(t)))
        pairs.append((a + extra, b) if t > 0 else (a, b + extra))
    return pairs


# ---------------------------------------------------------------- 1. the definition --
def test_definition_all_flag_combinations(ctx):
    """1 024 pairs up to 60 x 60, the 32 flag combinations, mixed-case DNA, w in 0 .. 12 per pair: both calls equal
    bandlib.expected; a batch with pairs that have no alignment inside their band returns E_TRACEBACK naming the lowest, and
    is correct without them."""
    rng = random.Random(4242)
    n_total = n_none = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        both_no_gaps = flags[2] and flags[3]
        init = [1, -6 if both_no_gaps else -2, -4, -1] if idx % 2 else [2, -7 if both_no_gaps else -3, 0, -2]
        sc = S.make_scoring({"init": [*init, *flags, 0]})
        osc = oracle_scoring_of(sc)
        pairs, bands = [], []
        for _ in range(32):
            la = rng.randrange(0, 61)
            a = bytes(rng.choice(b"ACGTacgt") for _ in range(la))
            if rng.random() < 0.8:
                b = BL.mutate(rng, a, 0.2, b"ACGTacgt")[:60]
            else:
                b = bytes(rng.choice(b"ACGTacgt") for _ in range(rng.randrange(0, 61)))
            pairs.append((a, b))
            bands.append(rng.randrange(0, 13))
        want = [BL.expected(osc, a, b, w) for (a, b), w in zip(pairs, bands)]
        want_score = [BL.expected_score(osc, a, b, w) for (a, b), w in zip(pairs, bands)]
        batch = W.from_pairs(pairs)
        score = ctx.nw_score_banded(batch, sc, bands)
        assert [int(s) for s in score] == want_score, (flags, init)
        none = [p for p, x in enumerate(want) if x is None]
        n_total += len(pairs)
        n_none += len(none)
        if none:
            assert all(want_score[p] < -2 ** 30 for p in none)
            with pytest.raises(S.SeqAlignError) as e:
                ctx.nw_align_banded(batch, sc, bands)
            assert e.value.code == S.E_TRACEBACK and f"pair {none[0]}:" in str(e.value), (str(e.value), none)
            keep = [p for p in range(len(pairs)) if want[p] is not None]
            pairs, bands, want = [pairs[p] for p in keep], [bands[p] for p in keep], [want[p] for p in keep]
            batch = W.from_pairs(pairs)
        got = both_calls(ctx, batch, sc, bands)
        bad = [(p, pairs[p], bands[p], got[p], want[p]) for p in range(len(pairs)) if got[p] != want[p]]
        assert not bad, (flags, init, bad[:2])
    assert n_total >= 1000 and n_none > 0, (n_total, n_none)


# ---------------------------------------------------------------- 2. a band that covers the matrix --
def test_whole_matrix_band_equals_the_unbanded_calls(ctx):
    n = 0
    for case in json.loads((GOLD / "fill_small.json").read_text())["cases"]:
        sc = S.make_scoring(case["scoring"])
        batch = W.from_pairs([(g["a"].encode(), g["b"].encode()) for g in case["pairs"]])
        assert int((batch.len_a + batch.len_b).max()) + 1 <= 1024
        got = both_calls(ctx, batch, sc, FULL)
        assert got == ctx.nw_batch(batch, sc), case["scoring"]
        assert [g[0] for g in got] == [int(s) for s in ctx.nw_score(batch, sc)]
        for p, g in enumerate(case["pairs"]):
            if "result_a" in g["nw"]:
                assert got[p] == (g["nw"]["score"], g["nw"]["result_a"].encode(), g["nw"]["result_b"].encode())
        n += batch.n_pairs
    assert n >= 100
    # C2's golden pairs (the compiled reference's results): every pair, byte for byte
    configs = json.loads((GOLD / "configs.json").read_text())
    for name in ("C2", "C2_related"):
        cfg = configs[name]
        sc = S.make_scoring(cfg["scoring"])
        batch = W.make(cfg["gen"], cfg["n"], cfg["kwargs"])
        assert batch.n_pairs == len(cfg["pairs"]) >= 64
        got = both_calls(ctx, batch, sc, FULL)
        assert got == ctx.nw_batch(batch, sc), name
        assert [g[0] for g in got] == [int(s) for s in ctx.nw_score(batch, sc)], name
        for p, g in enumerate(cfg["pairs"]):
            assert got[p] == (g["score"], g["result_a"].encode(), g["result_b"].encode()), (name, p)
    sc = S.make_scoring({"preset": "default"})
    osc = O.build_scoring({"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]}, "oracle")
    for batch in (W.dna_nw_150(64, seed=7), W.ragged(48, seed=11, max_len=500)):
        got = both_calls(ctx, batch, sc, FULL)
        assert got == ctx.nw_batch(batch, sc)
        assert [g[0] for g in got] == [int(s) for s in ctx.nw_score(batch, sc)]
        for p in (0, 17, batch.n_pairs - 1):
            rc, s, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and got[p] == (s, ra, rb)


# ---------------------------------------------------------------- 3. every frame class, both phases --
def frame_pairs():
    rng = random.Random(77)
    lengths = [30, 47, 64, 100, 150, 333, 640, 1000, 1500, 2200, 3100, 4000, 5000, 6000, 900, 1800, 2600, 3500, 700, 1300]
    tails = [0, 1, 0, 0, -3, 2, 0, 17, -40, 0, 101, -200, 0, 0, 500, -500, 333, -77, 250, -421]
    pairs = related_pairs(rng, lengths, tails=tails)
    same = bytes(rng.choice(b"ACGT") for _ in range(777))
    pairs += [(same, same), (b"", bytes(rng.choice(b"ACGT") for _ in range(40))), (bytes(rng.choice(b"ACGT") for _ in range(55)), b""),
              (b"", b""), (b"A", b"A")]
    return pairs


def in_band_runs(ctx, sc, pairs, widths):
    """Runs every pair with w0, w0 + 1, w0 + 37 and every w >= w0 that makes one of `widths`; each result must be nw_batch's.
    Returns the set of band widths that ran and w0 per pair."""
    batch = W.from_pairs(pairs)
    want = ctx.nw_batch(batch, sc)
    las, lbs = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    w0 = [BL.smallest_band(want[p][1], want[p][2], las[p], lbs[p]) for p in range(len(pairs))]
    for p in range(len(pairs)):
        assert BL.width_of(las[p], lbs[p], w0[p] + 37) <= 1024, (p, w0[p])          # no pair is left out for its width
    ran = set()

    def run(idx, bands):
        sub = W.from_pairs([pairs[p] for p in idx])
        got = both_calls(ctx, sub, sc, bands)
        bad = [(p, w, got[k][0], want[p][0]) for k, (p, w) in enumerate(zip(idx, bands)) if got[k] != want[p]]
        assert not bad, bad[:3]
        ran.update(BL.width_of(las[p], lbs[p], w) for p, w in zip(idx, bands))

    everyone = list(range(len(pairs)))
    for add in (0, 1, 37):
        run(everyone, [w0[p] + add for p in everyone])
    for width in widths:
        idx, bands = [], []
        for p in everyone:
            w = BL.w_for_width(las[p], lbs[p], width)
            if w is not None and w >= w0[p]:
                idx.append(p); bands.append(w)
        if idx:
            run(idx, bands)
    return ran, w0


def test_every_frame_class_and_both_phases(ctx):
    sc = S.make_scoring({"init": [*PLAIN, 0, 0, 0, 0, 0, 0]})
    pairs = frame_pairs()
    diffs = [len(a) - len(b) for a, b in pairs]
    assert max(diffs) >= 480 and min(diffs) <= -480 and any(len(a) == 0 for a, _ in pairs) and any(len(b) == 0 for _, b in pairs)
    ran, w0 = in_band_runs(ctx, sc, pairs, EDGE_WIDTHS)
    assert set(EDGE_WIDTHS) <= ran, sorted(set(EDGE_WIDTHS) - ran)      # both sides of every step of the ladder ran
    assert 1 in ran and 0 in w0                                         # identical pairs: one diagonal


@pytest.mark.parametrize("name", ["blosum62", "extend_pays", "no_end_gap", "no_start_no_end"])
def test_in_band_property_other_scorings(ctx, name):
    rng = random.Random(len(name))
    if name == "blosum62":
        sc = S.make_scoring({"preset": "BLOSUM62"})
        pairs = related_pairs(rng, [40, 90, 150, 260, 300, 333], b"ARNDCQEGHILKMFPSTWYV", tails=[0, 3, -5, 0, 30, -41])
    else:
        init = {"extend_pays": [3, -4, -9, 1, 0, 0, 0, 0, 0, 0], "no_end_gap": [1, -2, -4, -1, 0, 1, 0, 0, 0, 0],
                "no_start_no_end": [2, -3, -5, -2, 1, 1, 0, 0, 0, 0]}[name]
        sc = S.make_scoring({"init": init})
        pairs = related_pairs(rng, [30, 64, 100, 200, 310, 400], tails=[0, -2, 7, 0, -60, 45])
    ran, _ = in_band_runs(ctx, sc, pairs, [63, 64, 65, 128, 129, 256, 257, 512, 513])
    assert len(ran) >= 6


# ---------------------------------------------------------------- 4. the path outside the band --
def test_path_outside_the_band(ctx):
    sc = S.make_scoring({"init": [*PLAIN, 0, 0, 0, 0, 0, 0]})
    osc = oracle_scoring_of(sc)
    rng = random.Random(5)
    small = [(a, BL.mutate(rng, a, 0.25)) for a in (bytes(rng.choice(b"ACGT") for _ in range(n)) for n in [60, 90, 120, 140, 140, 100, 80, 130])]
    pairs = [(a, b[:150]) for a, b in small] + frame_pairs()
    batch = W.from_pairs(pairs)
    full = ctx.nw_batch(batch, sc)
    w0 = [BL.smallest_band(full[p][1], full[p][2], len(pairs[p][0]), len(pairs[p][1])) for p in range(len(pairs))]
    idx = [p for p in range(len(pairs)) if w0[p] >= 1]                # (w0 = 0: there is no narrower band)
    assert len(idx) >= 20 and sum(1 for p in idx if p < len(small)) >= 4
    sub = W.from_pairs([pairs[p] for p in idx])
    bands = [w0[p] // 2 for p in idx]
    got = both_calls(ctx, sub, sc, bands)
    full_score = ctx.nw_score(sub, sc)
    lower = 0
    for k, p in enumerate(idx):
        a, b = pairs[p]
        score, ra, rb = got[k]
        assert score <= int(full_score[k]), p
        lower += score < int(full_score[k])
        assert ra.replace(b"-", b"") == a and rb.replace(b"-", b"") == b and len(ra) == len(rb), p
        assert BL.in_band(ra, rb, len(a), len(b), bands[k]), p
        assert rescore(ra, rb, *PLAIN) == score, p
        if len(a) <= 150 and len(b) <= 150:
            assert got[k] == BL.expected(osc, a, b, bands[k]), p
    assert lower >= 1                                                  # the narrower band did cost something somewhere


# ---------------------------------------------------------------- 5. long --
def long_pair():
    rng = random.Random(100003)
    a = bytes(rng.choice(b"ACGT") for _ in range(100000))
    return a, BL.mutate(rng, a, 0.05)


def test_long_pair_equals_align_long(ctx):
    sc = S.make_scoring({"init": [*PLAIN, 0, 0, 0, 0, 0, 0]})
    a, b = long_pair()
    w = (1024 - abs(len(a) - len(b)) - 1) // 2
    assert w > 0 and BL.width_of(len(a), len(b), w) <= 1024
    batch = W.from_pairs([(a, b)])
    (want,) = ctx.nw_align_long(batch, sc)
    assert BL.in_band(want[1], want[2], len(a), len(b), w), (BL.excursion(want[1], want[2]), BL.band_of(len(a), len(b), w))
    (got,) = both_calls(ctx, batch, sc, w)
    assert got == want
    info = ctx.last_call()
    assert set(info) == {"band_score"}, info
    # a pair whose shape alone needs more than 1 024 diagonals
    wide = W.from_pairs([(a[:300], (b * 21)[:2000000])])
    for call in (ctx.nw_score_banded, ctx.nw_align_banded):
        with pytest.raises(S.SeqAlignError) as e:
            call(wide, sc, 0)
        assert e.value.code == S.E_TOO_LARGE and "pair 0:" in str(e.value)


# ---------------------------------------------------------------- 6. chunks, memory, unknown pairs --
def test_chunks_and_memory(ctx):
    sc = S.make_scoring({"preset": "default"})
    rng = random.Random(31)
    pairs = related_pairs(rng, [600] * 12)
    batch = W.from_pairs(pairs)
    want = both_calls(ctx, batch, sc, 20)
    with ctx.options(chunk_bytes=1 << 20):
        got = ctx.nw_align_banded(batch, sc, 20)
        info = ctx.last_call()
        assert info["band_fill"][0] >= 3 and info["band_fill"][1] == 12 and info["band_walk"] == (info["band_fill"][0], 12), info
        assert got == want
        big = W.from_pairs(related_pairs(rng, [600, 2400, 600]))
        with pytest.raises(S.SeqAlignError) as e:
            ctx.nw_align_banded(big, sc, [20, 100, 20])
        assert e.value.code == S.E_NOMEM and "pair 1:" in str(e.value) and "bytes" in str(e.value), str(e.value)
        digits = [int(t) for t in str(e.value).replace(",", " ").split() if t.isdigit()]
        assert any(d >= 12 * 2401 * 201 for d in digits), str(e.value)      # the bytes needed are named
        small_budget = [int(s) for s in ctx.nw_score_banded(big, sc, [20, 100, 20])]     # the score call holds no cells: it fits
    assert small_budget == [g[0] for g in ctx.nw_align_banded(big, sc, [20, 100, 20])]
    # the score call holds no cells: its chunks are cut by the sequences' bytes (two pairs of 2 x 200 000 bytes per MiB)
    # (equal lengths: one width class, so one launch per chunk)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(200000)) for _ in range(8)]
    longer = W.from_pairs([(a, a[:99999 + k] + b"N" + a[100000 + k:]) for k, a in enumerate(seqs)])
    one_chunk = ctx.nw_score_banded(longer, sc, 5)
    assert ctx.last_call()["band_score"] == (1, 8)
    with ctx.options(chunk_bytes=1 << 20):
        score = ctx.nw_score_banded(longer, sc, 5)
        assert ctx.last_call()["band_score"][0] >= 3 and ctx.last_call()["band_score"][1] == 8
    assert [int(s) for s in score] == [int(s) for s in one_chunk]


def test_time_hook_refuses_a_batch_of_several_chunks(ctx):
    """seqalign_band_score_time_ms times the launches of ONE chunk: a batch of more than 1 MiB at chunk_bytes = 1 MiB is
    SEQALIGN_E_ARG with the hook's own message; at the default budget it returns `repeats` positive times."""
    sc = S.make_scoring({"preset": "default"})
    batch = W.from_pairs([(b"ACGT" * 50, b"ACGTTACGTACGAT" * 14)] * 4000)   # 200 + 196 + 64 bytes per pair: 1.8 MB
    with ctx.options(chunk_bytes=1 << 20):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.band_score_time_ms(batch, sc, 10, repeats=3)
    assert err.value.code == S.E_ARG and "seqalign_band_score_time_ms: the batch does not fit one chunk" in str(err.value), str(err.value)
    ms = ctx.band_score_time_ms(batch, sc, 10, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms


def test_unknown_pair_inside_and_outside_the_band(ctx):
    """X (in seq_a) against Y (in seq_b) has no score; every other pair of letters has one."""
    sc = S.make_scoring({"preset": "DNA_hybridization",
                         "mutations": [["x", c, -1] for c in "acgt"] + [[c, "y", -1] for c in "acgt"]})
    a = b"ACGGTCATTG" * 60
    b = a[:290] + b"T" + a[290:]
    with_x = a[:300] + b"X" + a[301:]
    near = b[:302] + b"Y" + b[303:]                # row 303 against column 301: diagonal -2
    far = b[:20] + b"Y" + b[21:]                   # row 21 against column 301: diagonal 280
    good = (a, b)
    inside = W.from_pairs([good, good, (with_x, far), (with_x, near), good, (with_x, near)])
    with pytest.raises(S.SeqAlignError) as want:
        ctx.nw_score(inside, sc)
    assert want.value.code == S.E_UNKNOWN_PAIR and "pair 2:" in str(want.value)      # unbanded: X meets Y in both
    for call in (ctx.nw_score_banded, ctx.nw_align_banded):
        with pytest.raises(S.SeqAlignError) as got:
            call(inside, sc, 8)
        assert got.value.code == S.E_UNKNOWN_PAIR and "pair 3:" in str(got.value), str(got.value)
        assert str(got.value).split("] ")[-1] == str(want.value).split("] ")[-1].replace("pair 2:", "pair 3:")
    outside = W.from_pairs([good, (with_x, far), good])
    got = both_calls(ctx, outside, sc, 8)
    assert got[0] == got[2] and got[1][1].replace(b"-", b"") == with_x


# ---------------------------------------------------------------- 7. what ran --
def test_last_call_reports_the_band_kernels(ctx):
    sc = S.make_scoring({"preset": "default"})
    batch = W.dna_nw_150(100, seed=3, related=True)
    old = {S.lib().seqalign_kernel_kind_name(k).decode() for k in range(S.K_MAX)}
    ctx.nw_score_banded(batch, sc, 16)
    info = ctx.last_call()
    assert info == {"band_score": (1, 100)}, info
    ctx.nw_align_banded(batch, sc, 16)
    info = ctx.last_call()
    assert info == {"band_fill": (1, 100), "band_walk": (1, 100)} and not (set(info) & old), info
    ctx.nw_score(batch, sc)
    assert set(ctx.last_call()) == {"score_rows"}                           # the second record is cleared with the first
    mixed = W.from_pairs([(batch.seq_a(p), batch.seq_b(p)) for p in range(10)])
    bands = [0, 40, 100, 0, 1, 2, 3, 150, 31, 32]
    cpl = {min(c for c in (1, 2, 3, 4, 5, 6, 8, 12, 16) if 64 * c >= BL.width_of(int(mixed.len_a[p]), int(mixed.len_b[p]), bands[p]))
           for p in range(10)}
    assert len(cpl) >= 3
    ctx.nw_score_banded(mixed, sc, bands)                                   # one launch per width class
    assert ctx.last_call()["band_score"] == (len(cpl), 10), ctx.last_call()
