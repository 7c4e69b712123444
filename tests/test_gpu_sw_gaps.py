"""GPU tier: SW gap-run counts at any length -- seqalign_sw_gaps_batch (sa_sw_gaps.hip, sa_batch_score.hip).

Per pair (score, end_a, end_b, gap_runs_a, gap_runs_b) of the first hit of sw_batch(min_score = 1, max_hits = 1): sw_score's
three byte for byte and the numbers of maximal '-' runs in the hit's two strings.  Every case the oracle can hold compares all
five outputs with the runs counted in the oracle's strings (swgaplib.want_gaps); the pair of 66 000 x 66 000 is held to
sw_align_long's strings counted on the host.
"""
import itertools
import random

import numpy as np
import pytest

import denselib as D
import maglib as G
import orclib as O
import seqalign_amd as S
import spanlib as SP
import statlib as ST
import swgaplib as SG
import swstatlib as SS
import test_gpu_sw_stats as TS      # its shapes: width_pairs, rand_seq
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

MIB = 1 << 20   # the smallest chunk_bytes the option accepts


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def oracle_scoring_of(sc):
    return O.Scoring.from_buffer_copy(bytes(sc))


def flat(init4):
    return S.make_scoring({"init": list(init4) + [0] * 6})


def check(ctx, pairs, sc, tag="", want=None):
    """sw_gaps against the '-' runs of the oracle's strings and against sw_score byte for byte."""
    batch = W.from_pairs(pairs)
    res = ctx.sw_gaps(batch, sc)
    ran = ctx.last_call()
    assert [x.dtype for x in res] == [np.int32] + [np.uint32] * 4
    got = SG.got_gaps(res)
    want = want if want is not None else SG.want_gaps(oracle_scoring_of(sc), pairs)
    bad = [(p, len(pairs[p][0]), len(pairs[p][1]), got[p], want[p]) for p in range(len(pairs)) if got[p] != want[p]]
    assert not bad, (tag, len(bad), bad[:5], ran)
    score = ctx.sw_score(batch, sc)
    assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(res[:3], score)), tag
    return want, ran


# ---------------------------------------------------------------- 1. the definition --
# test_sw_gaps_argument_cpu.py's seven: the last three have a gap_extend that pays
INITS = {"dna": [1, -2, -4, -1], "open0": [2, -1, 0, -1], "ext0": [3, -1, -1, 0], "ties": [1, 0, 0, 0], "ext_pos": [2, -3, -2, 1],
         "ext_pos2": [3, -2, -3, 2], "ext_open0": [2, -3, -1, 1]}
EXT_POS = ("ext_pos", "ext_pos2", "ext_open0")
PROTEIN = b"ARNDCQEGHILKMFPSTWYV"


@pytest.mark.parametrize("name", list(INITS))
def test_small_pairs_dna_and_protein(ctx, name):
    """Pairs of 0 .. 40 letters, unrelated and related, over ACGT, the twenty amino acids and AC, and the zero lengths."""
    rng = random.Random(4100 + len(name))
    pairs = [(b"", b""), (b"ACGT", b""), (b"", b"ACGT"), (b"A", b"A"), (b"AAAA", b"CCCC")]
    for alpha in (b"ACGT", PROTEIN, b"AC"):
        for _ in range(40):
            a = TS.rand_seq(rng, rng.randint(1, 40), alpha)
            b = SP.indel_relative(rng, a, alpha)[:40] if rng.random() < 0.6 else TS.rand_seq(rng, rng.randint(1, 40), alpha)
            pairs.append((a, b or alpha[:1]))
    pairs += SG.gap_rich_pairs(4100 + len(name), 20, b"ACGT", 36)
    want, ran = check(ctx, pairs, flat(INITS[name]), name)
    assert set(ran) == {"score_rows"}, ran
    assert want[:3] == [SG.ZEROS] * 3 and want[3] == (INITS[name][0], 1, 1, 0, 0)
    assert sum(w[0] > 0 for w in want) >= 60 and sum(w[3] > 0 for w in want) >= 5 and sum(w[4] > 0 for w in want) >= 5
    assert all(len(x) == 0 for x in ctx.sw_gaps(W.from_pairs([]), flat(INITS[name])))


def test_all_flag_combinations_vs_oracle(ctx):
    """The 32 combinations of the reference's five flags (the GENERAL sweep), some with a gap_extend that pays."""
    gapped = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        ext = 1 if idx % 5 == 2 else -1
        spec = {"init": [1, mismatch, -4 if ext < 0 else -2, ext, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        batch = W.ragged(24, seed=700 + idx, max_len=40, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        pairs = [(batch.seq_a(p), batch.seq_b(p)) for p in range(batch.n_pairs)] + SG.gap_rich_pairs(300 + idx, 6, b"ACGTacgt", 36)
        want, _ = check(ctx, pairs, S.make_scoring(spec), f"flags={flags}")
        gapped += sum(w[3] + w[4] > 0 for w in want)
    assert gapped >= 32, gapped


def test_adjacent_runs_are_two(ctx):
    """An insertion directly against a deletion: one run in each string (the oracle's strings say so)."""
    a, b = D.alternation(31, 40, 0, D.matches_of("swdense"))
    want, _ = check(ctx, [(a, b)], S.make_scoring(D.SCORINGS["swdense"]), "alternation")
    assert want[0][3] > 1 and want[0][4] > 1, want


# ---------------------------------------------------------------- 2. every row class, the strips and their seams --
ROW_WIDTHS = (64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512)
STRIP_WIDTHS = (513, 1024, 1025, 1100, 1600)
WIDTH_SCORINGS = {"dna": [1, -2, -4, -1], "ext0": [3, -1, -1, 0], "ext_pos": [2, -3, -2, 1]}


def b_of(pairs, rng):
    """width_pairs with len_b of 40 .. 80."""
    return [(a, b[:rng.randint(40, 80)]) for a, b in pairs]


@pytest.mark.parametrize("name", list(WIDTH_SCORINGS))
def test_every_row_class_and_the_strips_then_ragged_in_chunks(ctx, name):
    """Each width alone (both sides of every step of the ladder 1 .. 6, 8 columns per lane; two, three and four strips), all in
    one ragged call, and that call at chunk_bytes = 1 MiB among enough further pairs for several chunks."""
    sc = flat(WIDTH_SCORINGS[name])
    rng = random.Random(9300 + len(name))
    ragged, want = [], []
    for la in ROW_WIDTHS + STRIP_WIDTHS:
        pairs = b_of(TS.width_pairs(rng, la), rng)[:6]
        w, ran = check(ctx, pairs, sc, f"{name} la={la}")
        assert ran == ({"score_rows": (1, len(pairs))} if la <= 512 else {"score_strips": (1, len(pairs))}), (la, ran)
        ragged += pairs
        want += w
    assert sum(w[0] > 0 for w in want) >= len(want) // 2
    order = list(range(len(ragged)))
    rng.shuffle(order)
    ragged, want = [ragged[k] for k in order], [want[k] for k in order]
    _, ran = check(ctx, ragged, sc, f"{name} ragged", want)
    assert set(ran) == {"score_rows", "score_strips"} and ran["score_strips"][0] == 1, ran
    filler = [(TS.rand_seq(rng, rng.randint(100, 300)), TS.rand_seq(rng, rng.randint(100, 300))) for _ in range(3000)]   # 1.4 MB
    half = len(ragged) // 2
    many = ragged[:half] + filler + ragged[half:]
    whole = SG.got_gaps(ctx.sw_gaps(W.from_pairs(many), sc))
    at_default = ctx.last_call()
    assert whole[:half] + whole[half + 3000:] == want
    assert whole[half:half + 3000:100] == SG.want_gaps(oracle_scoring_of(sc), filler[::100])
    with ctx.options(chunk_bytes=MIB):
        _, at_mib = check(ctx, many, sc, f"{name} 1 MiB", whole)
    assert at_mib["score_rows"][0] > at_default["score_rows"][0] and at_mib["score_strips"][0] > at_default["score_strips"][0] == 1, \
        (at_mib, at_default)


@pytest.mark.parametrize("width", (60, 700, 1100))
@pytest.mark.parametrize("name", EXT_POS)
def test_gap_extend_that_pays(ctx, name, width):
    """gap_extend > 0: runs that begin by extending out of a cell of score 0 (test_sw_gaps_argument_cpu.py shows on the oracle
    that counting open moves misses them), in rows and across strips."""
    rng = random.Random(width + len(name))
    pairs = [(a, b[:rng.randint(40, 80)]) for a, b in ST.tie_pairs(name if name in ST.TIE_SCORINGS else "ext_pos", width, 8, b"ACGT")]
    pairs += [(TS.rand_seq(rng, width), TS.rand_seq(rng, rng.randint(40, 80))) for _ in range(4)]
    want, ran = check(ctx, pairs, flat(INITS[name]), f"{name} {width}")
    assert set(ran) == ({"score_rows"} if width <= 512 else {"score_strips"}), ran
    assert sum(w[3] + w[4] > 0 for w in want) >= 6, want


@pytest.mark.parametrize("width", [700, 1100, 1600])
@pytest.mark.parametrize("name", list(SP.SEAM_SCORINGS))
def test_ties_at_a_strip_seam(ctx, name, width):
    """spanlib.seam_pairs: hits planted across a seam that leave the seam column out of a cell where gap_a and gap_b tie -- the
    two states bring different runs, and A > B there rests on the one bit the left strip hands on."""
    pairs = SP.seam_pairs(name, width)
    _, ran = check(ctx, pairs, flat(SP.SEAM_SCORINGS[name]), f"seam {name} {width}")
    assert ran == {"score_strips": (1, len(pairs))}, ran


@pytest.mark.parametrize("width", (64, 512, 1100))
@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_ties_follow_the_walkers_order(ctx, name, width):
    """statlib.tie_pairs: test_sw_gaps_argument_cpu.py asserts on the oracle that such pairs change their runs under the reversed
    priority, so a kernel with the wrong tie order cannot pass."""
    check(ctx, ST.tie_pairs(name, width), flat(ST.TIE_SCORINGS[name]), f"ties {name} {width}")


DENSE_SHAPES = ((60, 60), (190, 150), (320, 100), (512, 100), (513, 150), (1100, 150))


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", D.SW_SCORINGS)
def test_gap_dense_pairs(ctx, name, shape):
    """denselib's alternation, straddling (the dense hit across column 512) and spaced pairs."""
    la, lb = shape
    pairs = D.span_counted(la, lb, name) + D.span_seam(la, lb, name) + D.span_added(la, lb, name)
    want, ran = check(ctx, pairs, S.make_scoring(D.SCORINGS[name]), f"{name} {shape}")
    assert ran == ({"score_strips": (1, len(pairs))} if la > 512 else {"score_rows": (1, len(pairs))}), ran
    assert sum(w[3] for w in want) > 0 and sum(w[4] for w in want) > 0


# ---------------------------------------------------------------- 3. errors --
def test_unknown_character_pair_names_the_lowest_pair(ctx):
    """The span call's code and the span call's pair; narrow rows and strips alike; the context works afterwards."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    for width in (60, 1500):
        good = (b"ACGT" * (width // 4), b"TTACGTACGTACGA" * 5)
        pairs = [good] * 90
        pairs[61] = (good[0], good[1][:20] + b"X" + good[1][21:])
        pairs[40] = (good[0][:7] + b"X" + good[0][8:], good[1])
        batch = W.from_pairs(pairs)
        with pytest.raises(S.SeqAlignError) as ref:
            ctx.sw_span(batch, hyb)
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_gaps(batch, hyb)
        assert err.value.code == ref.value.code == S.E_UNKNOWN_PAIR
        assert str(err.value).replace("sw_gaps", "sw_span") == str(ref.value) and "pair 40:" in str(err.value)
        check(ctx, [good] * 5, hyb, f"after the failure, width {width}")


def test_one_scoring_on_each_side_of_the_domain_bound(ctx):
    """maglib's `steep` scoring on its 96 x 96 pairs: at the largest scale the documented rule admits the five outputs equal the
    oracle's; one scale further the call is SEQALIGN_E_DOMAIN, as the span call, and nothing is launched."""
    base = G.BASES["steep"]
    pairs = [G.pair("sq", kind) for kind in G.kinds_of("sq")]
    la, lb = max(len(a) for a, _ in pairs), max(len(b) for _, b in pairs)
    lo, hi = 1, 1 << 31
    while hi - lo > 1:                       # the rule is monotone in the scale
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if G.admitted(G.scaled(base, mid), la, lb, "score") else (lo, mid)
    inside, outside = G.scaled(base, lo), G.scaled(base, hi)
    want, _ = check(ctx, pairs, S.make_scoring(inside), f"steep x {lo}")
    assert max(w[0] for w in want) > 1 << 30
    ctx.sw_gaps(W.from_pairs(pairs[:1]), flat([1, -2, -4, -1]))
    with pytest.raises(S.SeqAlignError) as err:
        ctx.sw_gaps(W.from_pairs(pairs), S.make_scoring(outside))
    assert err.value.code == S.E_DOMAIN and str(G.INT32_MAX) in str(err.value), str(err.value)
    assert not ctx.last_call(), ctx.last_call()


def test_time_hook(ctx):
    sc = flat([1, -2, -4, -1])
    rng = random.Random(3131)
    pairs = [(TS.rand_seq(rng, rng.randint(100, 300)), TS.rand_seq(rng, rng.randint(100, 300))) for _ in range(100)]
    pairs += [(TS.rand_seq(rng, 1600), TS.rand_seq(rng, 133))]
    ms = ctx.sw_gaps_time_ms(W.from_pairs(pairs), sc, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms
    assert set(ctx.last_call()) == {"score_rows", "score_strips"}, ctx.last_call()
    filler = W.from_pairs([(b"ACGT" * 50, b"TTACGTACGTACGA" * 10)] * 4000)      # 1.6 MB
    with ctx.options(chunk_bytes=MIB):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_gaps_time_ms(filler, sc, repeats=2)
    assert err.value.code == S.E_ARG and "seqalign_sw_gaps_time_ms: the batch does not fit one chunk" in str(err.value)


# ---------------------------------------------------------------- 4. past 65 535 letters --
N = SG.LONG


def gapped(pair, at_b):
    """swstatlib.planted's pair with two letters inserted into and three deleted from seq_b inside the planted stretch."""
    a, b = pair
    return a, b[:at_b + 50] + b"KM" + b[at_b + 50:at_b + 120] + b[at_b + 123:]


LONG_CASES = {
    "end_a past 65 535": lambda rng: gapped(SS.planted(rng, N, 300, N - 230, 40, 200), 40),
    "end_b past 65 535": lambda rng: gapped(SS.planted(rng, 300, N, 60, N - 230, 200), N - 230),
}


@pytest.mark.parametrize("case", list(LONG_CASES))
def test_planted_gapped_hit_past_coordinate_65535(ctx, case):
    """66 000 x 300 and 300 x 66 000 (20 M cells: the oracle holds them) with a gapped hit past coordinate 65 535."""
    a, b = LONG_CASES[case](random.Random(len(case)))
    sc = flat([1, -2, -4, -1])
    want, ran = check(ctx, [(a, b)], sc, case)
    score, end_a, end_b, ga, gb = want[0]
    assert score > 100 and ga == 1 and gb == 1 and (end_a if "end_a" in case else end_b) > 65535, want
    assert set(ran) == ({"score_rows"} if len(a) <= 512 else {"score_strips"})


def test_deleted_block_past_65535_against_align_long(ctx):
    """66 000 x 65 960 (4.4e9 cells: no oracle holds them): a sequence against itself with one block of 40 deleted.  Held to the
    '-' runs of sw_align_long's strings counted on the host (test_sw_gaps_argument_cpu.py shows the construction on the oracle at
    400 letters)."""
    pair = SG.deleted_block(W.Rng(66000))
    sc = flat(SG.BLOCK_INIT)
    batch = W.from_pairs([pair])
    got = SG.got_gaps(ctx.sw_gaps(batch, sc))[0]
    assert set(ctx.last_call()) == {"score_strips"}
    assert tuple(int(x[0]) for x in ctx.sw_score(batch, sc)) == got[:3]
    hits, = ctx.sw_align_long(batch, sc, 1)
    assert SG.host_gaps(hits) == got, (SG.host_gaps(hits), got)
    assert got[1:] == (N, N - 40, 0, 1), got
