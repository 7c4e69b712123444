"""GPU tier: SW identity counts at any length -- seqalign_sw_counts_batch (sa_sw_counts.hip, sa_batch_score.hip).

Per pair (score, end_a, end_b, matches, mismatches) of the first hit of sw_batch(min_score = 1, max_hits = 1): sw_score's three
byte for byte and sw_stats' two counts, carried as two full words with no stop cell, so with no limit on the lengths.  Every
case below the 65 535-letter limit compares all five outputs with the oracle (swstatlib.want_sw_stats), with sw_score and with
sw_stats on the same batch; past the limit the oracle still holds 66 000 x 300, and the two pairs of 66 000 x 66 000 hold by
construction and are held to sw_align_long's hit besides.
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
import swcountlib as SC
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


def check(ctx, pairs, sc, tag="", want=None, stats=True):
    """sw_counts against the oracle, against sw_score byte for byte, and (stats) against sw_stats on the same batch."""
    batch = W.from_pairs(pairs)
    res = ctx.sw_counts(batch, sc)
    ran = ctx.last_call()
    assert [x.dtype for x in res] == [np.int32] + [np.uint32] * 4
    got = SC.got_counts(res)
    want = want if want is not None else SC.want_counts(oracle_scoring_of(sc), pairs)
    bad = [(p, len(pairs[p][0]), len(pairs[p][1]), got[p], want[p]) for p in range(len(pairs)) if got[p] != want[p]]
    assert not bad, (tag, len(bad), bad[:5], ran)
    score = ctx.sw_score(batch, sc)
    assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(res[:3], score)), tag
    if stats:
        assert got == [SC.counts_of(s) for s in SS.got_sw_stats(ctx.sw_stats(batch, sc))], tag
    return want, ran


# ---------------------------------------------------------------- 1. the definition --
INITS = {"dna": [1, -2, -4, -1], "open0": [2, -1, 0, -1], "ext0": [3, -1, -1, 0], "ties": [1, 0, 0, 0], "ext_pos": [2, -3, -2, 1]}
PROTEIN = b"ARNDCQEGHILKMFPSTWYV"


@pytest.mark.parametrize("name", list(INITS))
def test_small_pairs_dna_and_protein(ctx, name):
    """Pairs of 1 .. 40 letters, unrelated and related, over ACGT and over the twenty amino acids, and the zero lengths."""
    rng = random.Random(4100 + len(name))
    pairs = [(b"", b""), (b"ACGT", b""), (b"", b"ACGT"), (b"A", b"A"), (b"AAAA", b"CCCC")]
    for alpha in (b"ACGT", PROTEIN, b"AC"):
        for _ in range(40):
            a = TS.rand_seq(rng, rng.randint(1, 40), alpha)
            b = SP.indel_relative(rng, a, alpha)[:40] if rng.random() < 0.6 else TS.rand_seq(rng, rng.randint(1, 40), alpha)
            pairs.append((a, b or alpha[:1]))
    want, ran = check(ctx, pairs, flat(INITS[name]), name)
    assert set(ran) == {"score_rows"}, ran
    assert want[:3] == [SC.ZEROS] * 3 and want[3] == (INITS[name][0], 1, 1, 1, 0) and want[4] == SC.ZEROS
    assert sum(w[0] > 0 for w in want) >= 60 and sum(w[3] for w in want) > 0
    assert all(len(x) == 0 for x in ctx.sw_counts(W.from_pairs([]), flat(INITS[name])))


def test_all_flag_combinations_vs_oracle(ctx):
    """The 32 combinations of the reference's five flags (the GENERAL sweep): mixed case, wildcards and mutations play no part
    in the counts, case folding does."""
    mismatches = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        batch = W.ragged(24, seed=700 + idx, max_len=40, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        pairs = [(batch.seq_a(p), batch.seq_b(p)) for p in range(batch.n_pairs)]
        want, _ = check(ctx, pairs, S.make_scoring(spec), f"flags={flags}")
        mismatches += sum(w[4] for w in want)
    assert mismatches > 0


def test_case_folding_decides_the_bucket(ctx):
    a, b = b"ACGTACGTACGTACGTACGT", b"acgtacgtacgtacgtacgt"
    sc = S.make_scoring({"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]})      # folded: lower case matches upper case
    assert check(ctx, [(a, b), (a, a)], sc, "folded")[0] == [(20, 20, 20, 20, 0)] * 2
    # case sensitive with a mismatch score that pays: the lower-case letters are twenty mismatches of the same hit
    sc = S.make_scoring({"init": [1, 1, -4, -1, 0, 0, 0, 0, 0, 1]})
    assert check(ctx, [(a, b), (a, a)], sc, "case sensitive")[0] == [(20, 20, 20, 0, 20), (20, 20, 20, 20, 0)]


# ---------------------------------------------------------------- 2. every row class, the strips and their seams --
ROW_WIDTHS = (1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512)
STRIP_WIDTHS = (513, 1024, 1025, 1537)
WIDTH_SCORINGS = {"dna": [1, -2, -4, -1], "ext0": [3, -1, -1, 0], "ext_pos": [2, -3, -2, 1]}


def short_b(pairs, rng):
    """width_pairs with len_b about 40: seq_b cut to 30 .. 50 letters."""
    return [(a, b[:rng.randint(30, 50)]) for a, b in pairs]


@pytest.mark.parametrize("name", list(WIDTH_SCORINGS))
def test_every_row_class_and_the_strips_then_ragged_in_chunks(ctx, name):
    """Each width alone (both sides of every step of the ladder 1 .. 6, 8 columns per lane; two, three and four strips), all in
    one ragged call, and that call at chunk_bytes = 1 MiB among enough further pairs for several chunks."""
    sc = flat(WIDTH_SCORINGS[name])
    rng = random.Random(9300 + len(name))
    ragged, want = [], []
    for la in ROW_WIDTHS + STRIP_WIDTHS:
        pairs = short_b(TS.width_pairs(rng, la), rng)
        w, ran = check(ctx, pairs, sc, f"{name} la={la}")
        assert ran == ({"score_rows": (1, len(pairs))} if la <= 512 else {"score_strips": (1, len(pairs))}), (la, ran)
        ragged += pairs
        want += w
    assert sum(w[0] > 0 for w in want) >= len(want) // 2
    order = list(range(len(ragged)))
    rng.shuffle(order)
    ragged, want = [ragged[k] for k in order], [want[k] for k in order]
    _, ran = check(ctx, ragged, sc, f"{name} ragged", want)
    assert set(ran) == {"score_rows", "score_strips"} and ran["score_rows"][0] == 7 and ran["score_strips"][0] == 1, ran
    filler = [(TS.rand_seq(rng, rng.randint(100, 300)), TS.rand_seq(rng, rng.randint(100, 300))) for _ in range(3000)]   # 1.4 MB
    half = len(ragged) // 2
    many = ragged[:half] + filler + ragged[half:]
    whole = SC.got_counts(ctx.sw_counts(W.from_pairs(many), sc))
    at_default = ctx.last_call()
    assert whole[:half] + whole[half + 3000:] == want
    assert whole[half:half + 3000:100] == SC.want_counts(oracle_scoring_of(sc), filler[::100])
    with ctx.options(chunk_bytes=MIB):
        _, at_mib = check(ctx, many, sc, f"{name} 1 MiB", whole)
    assert at_mib["score_rows"][0] > at_default["score_rows"][0] and at_mib["score_strips"][0] > at_default["score_strips"][0] == 1, \
        (at_mib, at_default)


@pytest.mark.parametrize("width", [700, 1100, 1600])
@pytest.mark.parametrize("name", list(SP.SEAM_SCORINGS))
def test_ties_at_a_strip_seam(ctx, name, width):
    """spanlib.seam_pairs: hits planted across a seam that leave the seam column out of a cell where gap_a and gap_b tie -- the
    two states bring different counts, and A > B there rests on the one bit the left strip hands on."""
    pairs = SP.seam_pairs(name, width)
    _, ran = check(ctx, pairs, flat(SP.SEAM_SCORINGS[name]), f"seam {name} {width}")
    assert ran == {"score_strips": (1, len(pairs))}, ran


def test_equal_best_cells_in_two_strips(ctx):
    """The same stretch planted in strip 0 and in strip 2 of seq_a and once in seq_b: equal best cells in two strips.  The lower
    column wins (merge_left_best_span: a tie goes to the left strip) and the end cell shows which copy brought the counts."""
    rng = random.Random(77)
    core = TS.rand_seq(rng, 60, b"GT")
    a = bytearray(TS.rand_seq(rng, 1537, b"A"))
    a[100:160] = core
    a[1300:1360] = core
    b = bytes(TS.rand_seq(rng, 10, b"C")) + core + bytes(TS.rand_seq(rng, 10, b"C"))
    want, ran = check(ctx, [(bytes(a), b)], flat([1, -2, -4, -1]), "two strips")
    assert want == [(60, 160, 70, 60, 0)] and set(ran) == {"score_strips"}, (want, ran)


@pytest.mark.parametrize("width", (64, 512, 1100))
@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_ties_follow_the_walkers_order(ctx, name, width):
    """statlib.tie_pairs: test_sw_stats_argument_cpu.py asserts on the oracle that at least TIE_MIN of these change their counts
    under the reversed priority, so a kernel with the wrong tie order cannot pass."""
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
    assert sum(w[3] for w in want) > 0


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
            ctx.sw_counts(batch, hyb)
        assert err.value.code == ref.value.code == S.E_UNKNOWN_PAIR
        assert str(err.value).replace("sw_counts", "sw_span") == str(ref.value) and "pair 40:" in str(err.value)
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
    ctx.sw_counts(W.from_pairs(pairs[:1]), flat([1, -2, -4, -1]))
    with pytest.raises(S.SeqAlignError) as err:
        ctx.sw_counts(W.from_pairs(pairs), S.make_scoring(outside))
    assert err.value.code == S.E_DOMAIN and str(G.INT32_MAX) in str(err.value), str(err.value)
    assert not ctx.last_call(), ctx.last_call()


def test_time_hook(ctx):
    sc = flat([1, -2, -4, -1])
    rng = random.Random(3131)
    pairs = [(TS.rand_seq(rng, rng.randint(100, 300)), TS.rand_seq(rng, rng.randint(100, 300))) for _ in range(100)]
    pairs += [(TS.rand_seq(rng, 1600), TS.rand_seq(rng, 133))]
    ms = ctx.sw_counts_time_ms(W.from_pairs(pairs), sc, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms
    assert set(ctx.last_call()) == {"score_rows", "score_strips"}, ctx.last_call()
    filler = W.from_pairs([(b"ACGT" * 50, b"TTACGTACGTACGA" * 10)] * 4000)      # 1.6 MB
    with ctx.options(chunk_bytes=MIB):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_counts_time_ms(filler, sc, repeats=2)
    assert err.value.code == S.E_ARG and "seqalign_sw_counts_time_ms: the batch does not fit one chunk" in str(err.value)


# ---------------------------------------------------------------- 4. past 65 535 letters --
N = SC.LONG
LONG_CASES = {
    "end_a past 65 535": lambda rng: SS.planted(rng, N, 300, N - 230, 40, 200),
    "end_b past 65 535": lambda rng: SS.planted(rng, 300, N, 60, N - 230, 200),
}


def refuses_sw_stats(ctx, batch, sc):
    with pytest.raises(S.SeqAlignError) as err:
        ctx.sw_stats(batch, sc)
    assert err.value.code == S.E_TOO_LARGE and str(N) in str(err.value), str(err.value)


@pytest.mark.parametrize("case", list(LONG_CASES))
def test_planted_hit_past_coordinate_65535(ctx, case):
    """66 000 x 300 and 300 x 66 000 (20 M cells: the oracle holds them) with the hit past coordinate 65 535: the end needs more
    than 16 bits, sw_span's pos + len equals it, and sw_stats refuses the pair."""
    a, b = LONG_CASES[case](random.Random(len(case)))
    sc = flat([1, -2, -4, -1])
    want, ran = check(ctx, [(a, b)], sc, case, stats=False)
    score, end_a, end_b, m, mm = want[0]
    assert score > 150 and m > 150 and mm > 0 and (end_a if "end_a" in case else end_b) > 65535, want
    assert set(ran) == ({"score_rows"} if len(a) <= 512 else {"score_strips"})
    batch = W.from_pairs([(a, b)])
    span = [int(x[0]) for x in ctx.sw_span(batch, sc)]
    assert (span[0], span[1] + span[3], span[2] + span[4]) == (score, end_a, end_b), (span, want)
    refuses_sw_stats(ctx, batch, sc)


@pytest.mark.parametrize("case", ["matches", "mismatches"])
def test_counts_past_65535_by_construction_and_against_align_long(ctx, case):
    """66 000 x 66 000 (4.4e9 cells: no oracle holds them).  A sequence against itself under [1, -2, -4, -1]: 66 000 matches;
    A...A against C...C under [1, 1, -4, -1]: the hit is the whole diagonal, 66 000 mismatches.  Both hold by construction
    (test_sw_counts_argument_cpu.py shows the construction on the oracle at 300 letters) and are held to sw_align_long's hit
    with its strings counted on the host."""
    if case == "matches":
        pair, sc, expect = SC.self_pair(W.Rng(66000)), flat(SC.SELF_INIT), (N, N, N, N, 0)
    else:
        pair, sc, expect = SC.apart_pair(), flat(SC.APART_INIT), (N, N, N, 0, N)
    batch = W.from_pairs([pair])
    got = SC.got_counts(ctx.sw_counts(batch, sc))[0]
    assert set(ctx.last_call()) == {"score_strips"}
    assert got == expect, (got, expect)
    assert tuple(int(x[0]) for x in ctx.sw_score(batch, sc)) == expect[:3]
    hits, = ctx.sw_align_long(batch, sc, 1)
    assert SC.host_counts(oracle_scoring_of(sc), hits) == got
    refuses_sw_stats(ctx, batch, sc)
