"""GPU tier: banded NW statistics -- seqalign_nw_stats_banded (sa_band_nw_stats.hip, sa_batch_band.hip).

Every result is checked three ways (check): bit for bit against the oracle -- the banded end value and the counted columns of
its walk over the banded matrices (bandnwstatlib.want), or SEQALIGN_E_TRACEBACK naming the lowest pair that has no
alignment inside its band; the score against ctx.nw_score_banded on the same batch; and all three values against ctx.nw_stats for every pair
whose band is the whole matrix.  Shapes are the smallest at which the frame can go wrong: len_b >= -d_lo + 70, so that the frame
moves across a 64-row code fetch; every width at which the columns per lane step up, both sides of it; len_a above, below and
beside len_b; the alignment along the band's left edge, its right edge and its middle."""
import itertools
import random

import numpy as np
import pytest

import bandlib as BL
import bandnwstatlib as BN
import bandspanlib as BSP
import orclib as O
import seqalign_amd as S
import statlib as ST
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

PLAIN = [1, -2, -4, -1]
FULL = 2 ** 32 - 1
LADDER = [64, 128, 192, 256, 320, 384, 512]          # widths at which the columns per lane step up: 1 .. 6, 8
WIDTHS = [1, 2, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 511, 512]
MIB = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def scoring(init4, **flags):
    sc = S.make_scoring(ST.init_spec(init4, **flags))
    return sc, O.Scoring.from_buffer_copy(bytes(sc))


def class_of(width):
    return next(k for k, top in enumerate(LADDER) if width <= top)


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def check(ctx, sc, osc, triples, want=None):
    """The statistics call on [(a, b, w)] the three ways of the module's header; returns the wanted list (None: no alignment
    inside the band).  A batch with such pairs must raise E_TRACEBACK naming the lowest, and is checked without them."""
    want = want or [BN.want(osc, a, b, w) for a, b, w in triples]
    none = [p for p, x in enumerate(want) if x is None]
    if none:
        with pytest.raises(S.SeqAlignError) as e:
            ctx.nw_stats_banded(W.from_pairs([(a, b) for a, b, _ in triples]), sc, [w for _, _, w in triples])
        assert e.value.code == S.E_TRACEBACK and f"pair {none[0]}:" in str(e.value), (str(e.value), none)
    kept = [p for p, x in enumerate(want) if x is not None]
    if not kept:
        return want
    batch = W.from_pairs([triples[p][:2] for p in kept])
    bands = [triples[p][2] for p in kept]
    res = ctx.nw_stats_banded(batch, sc, bands)
    assert [r.dtype for r in res] == [np.int32, np.uint32, np.uint32] and all(r.shape == (len(kept),) for r in res)
    got = ST.got_stats(res)
    bad = [(p, triples[p][2], got[k], want[p]) for k, p in enumerate(kept) if got[k] != want[p]]
    assert not bad, (len(bad), bad[:3])
    assert np.array_equal(res[0], ctx.nw_score_banded(batch, sc, bands))
    whole = [k for k, p in enumerate(kept)
             if BL.width_of(len(triples[p][0]), len(triples[p][1]), triples[p][2]) == len(triples[p][0]) + len(triples[p][1]) + 1]
    if whole:
        full = ST.got_stats(ctx.nw_stats(W.from_pairs([triples[kept[k]][:2] for k in whole]), sc))
        assert full == [got[k] for k in whole]
    return want


# ---------------------------------------------------------------- 1. widths --
WIDTH_SCORINGS = {"ext0": ([3, -1, -1, 0], b"ARNDCQEGHILKMFPSTWYV"), "dna": (PLAIN, b"ACGT")}


def width_triples(rng, width, alpha):
    """Three pairs whose band is `width` diagonals wide, len_b >= -d_lo + 70:
    0: len_a > len_b, a core shared on the band's LOWEST diagonal (seq_b starts with w letters of its own, seq_a ends with the
       rest), swept while the frame moves;
    1: len_a < len_b, a shared prefix on diagonal 0 that outlasts the border column, then a core on the band's HIGHEST diagonal;
    2: lengths equal or one apart, a relative with 8 % edits: the middle.
    Where the width leaves no room (1, 2) the difference in length shrinks to what its parity needs."""
    spare = width - 1
    d0 = min(spare, 7 if spare % 2 else 6)                # |len_a - len_b| of pairs 0 and 1: width = d0 + 1 + 2 w
    out = []
    # 0: the left edge
    w = (spare - d0) // 2
    core = rand_seq(rng, rng.randrange(75, 95), alpha)
    out.append((core + rand_seq(rng, d0 + w, alpha), rand_seq(rng, w, alpha) + core, w))
    # 1: the right edge
    prefix, core = rand_seq(rng, d0 + w + 10, alpha), rand_seq(rng, rng.randrange(75, 95), alpha)
    out.append((prefix + rand_seq(rng, w, alpha) + core, prefix + core + rand_seq(rng, w + d0, alpha), w))
    # 2: the middle
    d2 = spare % 2
    w = (spare - d2) // 2
    a = rand_seq(rng, w + 75 + rng.randrange(20), alpha)
    b = BL.mutate(rng, a, 0.08, alpha)
    b = (b + rand_seq(rng, len(a), alpha))[:len(a) + d2]
    out.append((a, b, w))
    for a, b, w in out:
        d_lo, _ = BL.band_of(len(a), len(b), w)
        assert BL.width_of(len(a), len(b), w) == width and len(b) >= -d_lo + 70, (width, len(a), len(b), w)
    return out


@pytest.mark.parametrize("name", list(WIDTH_SCORINGS))
@pytest.mark.parametrize("width", WIDTHS)
def test_every_width_class_and_its_edges(ctx, width, name):
    init, alpha = WIDTH_SCORINGS[name]
    sc, osc = scoring(init)
    triples = width_triples(random.Random(1000 + width), width, alpha)
    if width > 2:
        assert len(triples[0][0]) > len(triples[0][1]) and len(triples[1][0]) < len(triples[1][1])
    both = [BN.want_walked(osc, a, b, w) for a, b, w in triples]
    if name == "ext0" and width > 2:                        # on the oracle alone: the alignments do run along the edges
        for (a, b, w), (three, walked), edge in zip(triples[:2], both[:2], (0, 1)):
            assert BL.excursion(walked[1], walked[2])[edge] == BL.band_of(len(a), len(b), w)[edge], (width, edge)
    want = check(ctx, sc, osc, triples, [three for three, walked in both])
    assert all(x[1] >= 60 for x in want[:2]) and (width < 64 or want[2][1] >= 60), want      # the cores; the relative


def test_an_alignment_that_leaves_the_band(ctx):
    """Relatives with 25 % edits at half the band their unbanded alignment needs: the banded result differs from nw_stats' on
    some pair, and is the oracle's."""
    sc, osc = scoring(PLAIN)
    rng = random.Random(5)
    pairs = [(a, BL.mutate(rng, a, 0.25)[:150]) for a in (rand_seq(rng, n) for n in [60, 90, 120, 140, 140, 100, 80, 130])]
    triples = []
    for a, b in pairs:
        rc, s, ra, rb = O.oracle_nw(osc, a, b)
        triples.append((a, b, BL.smallest_band(ra, rb, len(a), len(b)) // 2))
    want = check(ctx, sc, osc, triples)
    unbanded = ST.want_stats(osc, pairs)
    differ = [p for p in range(len(pairs)) if want[p] != unbanded[p]]
    assert differ and all(want[p][0] < unbanded[p][0] for p in differ), (want, unbanded)


# ---------------------------------------------------------------- 2. the whole matrix, empties --
def test_the_whole_matrix_as_band_is_the_unbanded_call(ctx):
    rng = random.Random(77)
    sc, osc = scoring(PLAIN)
    pairs = []
    for k in range(24):
        la = rng.randrange(1, 250)
        a = rand_seq(rng, la)
        b = BL.mutate(rng, a, 0.15)[:511 - la] if k % 3 else rand_seq(rng, rng.randrange(1, 512 - la))
        pairs.append((a, b))
    assert all(len(a) + len(b) + 1 <= 512 for a, b in pairs) and max(len(a) + len(b) for a, b in pairs) >= 400
    batch = W.from_pairs(pairs)
    want = check(ctx, sc, osc, [(a, b, FULL) for a, b in pairs])
    assert want == ST.want_stats(osc, pairs)
    got, full = ctx.nw_stats_banded(batch, sc, FULL), ctx.nw_stats(batch, sc)
    assert len(got) == len(full) == 3 and all(np.array_equal(g, f) and g.dtype == f.dtype for g, f in zip(got, full))


@pytest.mark.parametrize("no_start", [0, 1])
def test_empty_sequences_and_a_band_of_one_diagonal(ctx, no_start):
    sc, osc = scoring(PLAIN, no_start=no_start)
    a, b = b"ACGTTGCAAGCTTGCA" * 3, b"GGACGTTGCAAGCTTGCATT" * 2
    triples = [(b"", b, 0), (a, b"", 0), (b"", b"", 0), (b"", b, 9), (a, b"", FULL), (b"", b"", 5),
               (a, a, 0), (a, a[:21] + b"T" + a[22:], 0), (a, b, 0), (b, a, 0), (b"A", b"A", 0), (b"A", b"C", 0), (b"A", b"CC", 0)]
    want = check(ctx, sc, osc, triples)
    edge = (lambda n: 0) if no_start else (lambda n: -4 - n)
    assert want[:6] == [(edge(len(b)), 0, 0), (edge(len(a)), 0, 0), (0, 0, 0), (edge(len(b)), 0, 0), (edge(len(a)), 0, 0), (0, 0, 0)]
    assert want[6] == (len(a), len(a), 0) and want[7] == (len(a) - 3, len(a) - 1, 1)
    assert want[10] == (1, 1, 0) and want[11] == (-2, 0, 1)


# ---------------------------------------------------------------- 3. flags --
@pytest.mark.parametrize("idx", range(32))
def test_all_flag_combinations_at_width_70(ctx, idx):
    """bandnwstatlib.flag_pairs: 40 mixed-case pairs; what each batch loses to E_TRACEBACK is bounded on the oracle in
    test_nw_stats_banded_argument_cpu.py.  check() asserts the error and the lowest pair, then the batch without them."""
    flags = list(itertools.product([0, 1], repeat=5))[idx]
    spec = BSP.flag_scoring(idx, flags)
    sc = S.make_scoring(spec)
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    triples = BN.flag_pairs(idx, flags, b"ACGTacgt" + (b"N" if spec["wildcards"] else b""))
    want = check(ctx, sc, osc, triples)
    lost = sum(x is None for x in want)
    assert lost <= BN.FLAG_N // 4 and (lost == 0 or flags[2] or flags[3] or flags[4]), (flags, lost)


@pytest.mark.parametrize("flag", BN.ROW_FLAGS)
def test_flags_that_change_the_row_at_eight_columns_per_lane(ctx, flag):
    """Width 385 (w = 192 on equal lengths, 191 two apart), 275 .. 300 rows.  len_a > d_hi, so the band's right edge meets the
    last column (row len_a - d_hi): under no_end_gap_penalty gap_a of that cell reads the cell above -- outside the band --
    through D."""
    sc, osc = scoring(PLAIN, **{flag: 1})
    triples = BN.row_flag_triples(flag)
    want = check(ctx, sc, osc, triples)
    assert sum(x is not None for x in want) >= 3, want


# ---------------------------------------------------------------- 4. ties --
@pytest.mark.parametrize("w", BN.TIE_BANDS)
@pytest.mark.parametrize("width", BN.TIE_WIDTHS)
@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_inside_a_band(ctx, name, width, w):
    """bandnwstatlib.tie_batch; that each batch and band holds a pair whose wanted counts change under the reversed priority is
    asserted on the oracle in test_nw_stats_banded_argument_cpu.py."""
    sc, osc = scoring(ST.TIE_SCORINGS[name])
    want = check(ctx, sc, osc, [(a, b, w) for a, b in BN.tie_batch(name, width)])
    assert None not in want


# ---------------------------------------------------------------- 5. more scorings --
@pytest.mark.parametrize("name", ["blosum62", "extend_pays"])
def test_more_scorings(ctx, name):
    rng = random.Random(len(name))
    if name == "blosum62":
        sc, alpha = S.make_scoring({"preset": "BLOSUM62"}), b"ARNDCQEGHILKMFPSTWYV"
    else:
        sc, alpha = S.make_scoring({"init": [3, -4, -9, 1, 0, 0, 0, 0, 0, 0]}), b"ACGT"
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    triples = []
    for n, tail, w in ((40, 0, 3), (90, 3, 10), (150, -5, 40), (260, 0, 100), (300, 30, 12), (333, -41, 60)):
        a = rand_seq(rng, n, alpha)
        b = BL.mutate(rng, a, 0.08, alpha)
        extra = rand_seq(rng, abs(tail), alpha)
        triples.append((a + extra, b, w) if tail > 0 else (a, b + extra, w))
    assert len({class_of(BL.width_of(len(a), len(b), w)) for a, b, w in triples}) >= 3
    want = check(ctx, sc, osc, triples)
    assert None not in want and sum(x[2] > 0 for x in want) >= 3


# ---------------------------------------------------------------- 6. long --
def test_one_long_band(ctx):
    """3 000 x 2 999 at width 512 with 8 % edits: dozens of code fetches, the frame moving on all but 257 rows."""
    rng = random.Random(88)
    sc, osc = scoring(PLAIN)
    a = rand_seq(rng, 3000)
    b = (BL.mutate(rng, a, 0.08) + rand_seq(rng, 200))[:2999]
    assert BL.width_of(3000, 2999, 255) == 512
    (want,) = check(ctx, sc, osc, [(a, b, 255)])
    assert want[1] > 2500 and want[2] > 20, want


def test_counts_past_65535(ctx):
    """70 000 x 70 000 at w = 8; seq_b is seq_a with 700 planted substitutions and no indels.  With a gap at -11 and more, a
    mismatch at -1 and 17 diagonals to move in, the main diagonal is the unique optimum: by formula.  The oracle's whole
    matrices do not fit at this size; the GPU's own align call and a count of its strings stand in for it."""
    rng = random.Random(70000)
    n, k = 70000, 700
    sc, osc = scoring([1, -1, -10, -1])
    a = bytearray(rand_seq(rng, n))
    b = bytearray(a)
    for at in rng.sample(range(n), k):
        b[at] = b"ACGT"[(b"ACGT".index(b[at]) + 1 + rng.randrange(3)) % 4]
    a, b = bytes(a), bytes(b)
    assert sum(x != y for x, y in zip(a, b)) == k
    batch = W.from_pairs([(a, b)])
    got = ST.got_stats(ctx.nw_stats_banded(batch, sc, 8))
    assert got == [(n - 2 * k, n - k, k)], got
    assert int(ctx.nw_score_banded(batch, sc, 8)[0]) == n - 2 * k
    ((score, ra, rb),) = ctx.nw_align_banded(batch, sc, 8)
    assert (score,) + ST.count_columns(osc, ra, rb) == got[0]


# ---------------------------------------------------------------- 7. mixed classes and chunks --
def test_mixed_classes_in_one_call_and_in_three_chunks(ctx):
    """60 pairs from all seven width classes.  36 of them are a sequence of 30 000 letters against itself -- score 30 000,
    30 000 matches -- so that at chunk_bytes = 1 MiB, where a pair takes len_a + len_b + 72 bytes, the batch of 2.2 MB is cut
    into three chunks; the others are checked against the oracle."""
    rng = random.Random(9)
    sc, osc = scoring(PLAIN)
    widths = [1, 64, 65, 128, 129, 192, 201, 256, 301, 320, 351, 384, 401, 511, 3]
    triples, want = [], []
    for k in range(60):
        width = widths[k % len(widths)]
        if k % 5 in (1, 2, 3):
            a = rand_seq(rng, 30000)
            triples.append((a, a, (width - 1) // 2))        # equal lengths: an even width becomes the odd one below it
            want.append((30000, 30000, 0))
        else:
            d = 1 - width % 2                               # len_b - len_a: width = d + 1 + 2 w
            w = (width - 1 - d) // 2
            a = rand_seq(rng, w + rng.randrange(75, 100))
            triples.append((a, (BL.mutate(rng, a, 0.08) + rand_seq(rng, len(a)))[:len(a) + d], w))
            assert BL.width_of(len(a), len(a) + d, w) == width
            want.append(BN.want(osc, *triples[-1]))
    classes = [class_of(BL.width_of(len(a), len(b), w)) for a, b, w in triples]
    assert set(classes) == set(range(len(LADDER)))
    batch, bands = W.from_pairs([t[:2] for t in triples]), [t[2] for t in triples]
    one = ctx.nw_stats_banded(batch, sc, bands)
    assert ctx.last_call() == {"band_score": (7, 60)}
    assert ST.got_stats(one) == want
    assert np.array_equal(one[0], ctx.nw_score_banded(batch, sc, bands))
    # the greedy cut of the contract: a chunk closes before the pair that would take it over the budget
    chunks, used = [[]], 0
    for k, (a, b, w) in enumerate(triples):
        need = len(a) + len(b) + 72
        if chunks[-1] and used + need > MIB:
            chunks.append([])
            used = 0
        chunks[-1].append(k)
        used += need
    assert len(chunks) == 3
    with ctx.options(chunk_bytes=MIB):
        got = ctx.nw_stats_banded(batch, sc, bands)
        info = ctx.last_call()
    assert info == {"band_score": (sum(len({classes[k] for k in c}) for c in chunks), 60)}, info
    assert all(np.array_equal(g, o) for g, o in zip(got, one))


# ---------------------------------------------------------------- 8. errors --
def test_unknown_pair_inside_and_outside_the_band(ctx):
    """X (in seq_a) against Y (in seq_b) has no score; every other pair of letters has one."""
    sc = S.make_scoring({"preset": "DNA_hybridization",
                         "mutations": [["x", c, -1] for c in "acgt"] + [[c, "y", -1] for c in "acgt"]})
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    rng = random.Random(3)
    a = rand_seq(rng, 180)
    b = a[:90] + b"T" + a[90:]
    with_x = a[:100] + b"X" + a[101:]
    near, far = b[:103] + b"Y" + b[104:], b[:20] + b"Y" + b[21:]      # X meets Y on diagonal 100 - 103, or 100 - 20
    good = (a, b)
    assert BL.fill_unknown(osc, with_x, near, BL.band_of(180, 181, 8))[3] == [(101, 104)]
    assert BL.fill_unknown(osc, with_x, far, BL.band_of(180, 181, 8))[3] == []
    inside = W.from_pairs([good, good, (with_x, far), (with_x, near), good, (with_x, near)])
    with pytest.raises(S.SeqAlignError) as got:
        ctx.nw_stats_banded(inside, sc, 8)
    assert got.value.code == S.E_UNKNOWN_PAIR and "pair 3:" in str(got.value), str(got.value)
    want = check(ctx, sc, osc, [(*good, 8), (with_x, far, 8), (*good, 8)])
    assert None not in want and want[0] == want[2]


def test_the_lowest_failing_pair_decides_between_traceback_and_unknown_pair(ctx):
    """A table scoring that forbids mismatches and both kinds of gap: a pair with one substitution has no alignment inside
    any band (E_TRACEBACK); a pair in which Z meets Z inside the band has no score (E_UNKNOWN_PAIR: under no_mismatches only
    two EQUAL letters are looked up in the table, and it has no Z).  The lower pair's code is the call's, as in
    seqalign_nw_stats_batch."""
    sc = S.make_scoring({"preset": "DNA_hybridization",
                         "flags": {"no_mismatches": True, "no_gaps_in_a": True, "no_gaps_in_b": True}})
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    bandless = BN.bandless_pair(120, 60)
    a = bandless[0]
    unknown = (a[:50] + b"Z" + a[51:], a[:50] + b"Z" + a[51:])
    good = (a, a)
    assert BN.want(osc, *good, 8) == (BN.want(osc, *good, 8)[0], 120, 0) and BN.want(osc, *bandless, 8) is None
    assert BL.fill_unknown(osc, *unknown, BL.band_of(120, 120, 8))[3] == [(51, 51)]
    for pairs, code, pair in (([good, bandless, unknown], S.E_TRACEBACK, 1), ([good, unknown, bandless], S.E_UNKNOWN_PAIR, 1),
                              ([unknown], S.E_UNKNOWN_PAIR, 0), ([good, good, bandless], S.E_TRACEBACK, 2)):
        with pytest.raises(S.SeqAlignError) as got:
            ctx.nw_stats_banded(W.from_pairs(pairs), sc, 8)
        assert got.value.code == code and f"pair {pair}:" in str(got.value), (str(got.value), code, pair)
    check(ctx, sc, osc, [(*good, 8), (*good, 0)])


# ---------------------------------------------------------------- 9. random, and the GPU's own align call --
def test_seeded_random_pairs_bands_and_scorings(ctx):
    """300 pairs up to 200 x 200 in five batches, each under a plain scoring drawn at random, a random w per pair."""
    rng = random.Random(20240)
    n = 0
    for _ in range(5):
        match, ext = rng.randrange(1, 6), rng.randrange(-3, 1)
        sc, osc = scoring([match, rng.randrange(-6, 0), rng.randrange(-8, 1), ext])
        triples = []
        for k in range(60):
            la = rng.randrange(0, 201)
            a = rand_seq(rng, la)
            b = BL.mutate(rng, a, rng.uniform(0.02, 0.3))[:200] if k % 4 else rand_seq(rng, rng.randrange(0, 201))
            triples.append((a, b, rng.choice([0, 1, 2, 5, 17, 40, 100, rng.randrange(0, 156)])))
        assert all(BL.width_of(len(a), len(b), w) <= 512 for a, b, w in triples)
        want = check(ctx, sc, osc, triples)
        assert None not in want
        n += len(want)
    assert n == 300


def test_agrees_with_the_align_call_on_the_gpu(ctx):
    rng = random.Random(1313)
    sc, osc = scoring(PLAIN)
    pairs, bands = [], []
    for _ in range(200):
        a = rand_seq(rng, rng.randrange(1, 400))
        pairs.append((a, BL.mutate(rng, a, rng.uniform(0.02, 0.2))))
        bands.append(rng.randrange(0, 60))
    batch = W.from_pairs(pairs)
    got = ST.got_stats(ctx.nw_stats_banded(batch, sc, bands))
    aligned = ctx.nw_align_banded(batch, sc, bands)
    assert got == [(score,) + ST.count_columns(osc, ra, rb) for score, ra, rb in aligned]
    assert sum(g[2] > 0 for g in got) >= 150


# ---------------------------------------------------------------- 10. timing hook --
def test_time_hook_times_one_chunk_and_refuses_two(ctx):
    sc, _ = scoring(PLAIN)
    batch = W.from_pairs([(b"ACGT" * 50, b"ACGTTACGTACGAT" * 14)] * 4000)   # 200 + 196 + 72 bytes per pair: 1.9 MB
    with ctx.options(chunk_bytes=MIB):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.nw_stats_band_time_ms(batch, sc, 10, repeats=3)
    assert err.value.code == S.E_ARG and "seqalign_nw_stats_band_time_ms: the batch does not fit one chunk" in str(err.value), str(err.value)
    ms = ctx.nw_stats_band_time_ms(batch, sc, 10, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms
