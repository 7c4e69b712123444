"""GPU tier: SW statistics matrices -- seqalign_sw_stats_cross (sa_batch_score_cross.hip, the CROSS form of sa_sw_stats.hip).

The seven [n_queries][n_targets] matrices must be what sw_stats returns on the explicit Q x T batch (pos_a / len_a in the query),
which tests/test_gpu_sw_stats.py holds to the oracle; the scores and spans are checked against the oracle here too."""
import random
import re

import numpy as np
import pytest

import orclib as O
import seqalign_amd as S
import swstatlib as SS
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

MIB = 1 << 20
AMINO = b"ARNDCQEGHILKMFPSTWYV"


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def rand_seq(rng, n, alpha=AMINO):
    return bytes(rng.choice(alpha) for _ in range(n))


def relative(rng, s, alpha=AMINO):
    out = bytearray()
    for ch in s:
        r = rng.randrange(14)
        if r == 0:
            continue
        if r == 1:
            out += rand_seq(rng, rng.randint(1, 3), alpha)
        out.append(rng.choice(alpha) if r == 2 else ch)
    return bytes(out)


def check_cross(ctx, queries, targets, sc, tag, oracle_sample=8):
    q, t = W.seqset_from(queries), W.seqset_from(targets)
    got = ctx.sw_stats_cross(q, t, sc)
    ran = ctx.last_call()
    shape = (len(queries), len(targets))
    assert all(g.shape == shape for g in got) and got[0].dtype == np.int32 and all(g.dtype == np.uint32 for g in got[1:])
    want = tuple(x.reshape(shape) for x in ctx.sw_stats(W.cross_batch(q, t), sc))
    for name, g, w in zip(("score", "pos_a", "pos_b", "len_a", "len_b", "matches", "mismatches"), got, want):
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist())
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    rng = random.Random(len(tag))
    for _ in range(oracle_sample):
        qi, ti = rng.randrange(shape[0]), rng.randrange(shape[1])
        assert tuple(int(g[qi, ti]) for g in got) == SS.want_one(osc, queries[qi], targets[ti]), (tag, qi, ti)
    return got, ran


def test_ragged_protein_cross_equals_the_explicit_batch(ctx):
    """7 x 9 ragged proteins under BLOSUM62, relatives among them, a target of length 0."""
    rng = random.Random(79)
    sc = S.make_scoring({"preset": "BLOSUM62"})
    queries = [rand_seq(rng, n) for n in (30, 64, 65, 129, 200, 333, 512)]
    targets = [rand_seq(rng, n) for n in (1, 50, 140, 300)] + [b""] + [relative(rng, queries[k]) for k in (1, 3, 5, 6)]
    got, ran = check_cross(ctx, queries, targets, sc, "7x9")
    assert set(ran) == {"score_cross"}, ran
    assert all(int(g[:, 4].max()) == 0 for g in got)                       # the empty target: seven zeros
    assert int(got[5].sum()) > 0 and int(got[6].sum()) > 0
    assert (got[5] + got[6] <= np.minimum(got[3], got[4])).all()


def test_long_queries_take_the_strips_route(ctx):
    """One query of 700 and one of 1 100 columns among short ones: their rows run the strips on explicit pair slices, the others
    the cross kernel."""
    rng = random.Random(1100)
    sc = S.make_scoring({"preset": "BLOSUM62"})
    queries = [rand_seq(rng, 90), rand_seq(rng, 700), rand_seq(rng, 40), rand_seq(rng, 1100), rand_seq(rng, 513), rand_seq(rng, 512)]
    targets = [rand_seq(rng, 120), b"", relative(rng, queries[1][300:650]), relative(rng, queries[3][400:800]), rand_seq(rng, 77),
               relative(rng, queries[3][900:]), relative(rng, queries[0])]
    got, ran = check_cross(ctx, queries, targets, sc, "strips route", oracle_sample=12)
    assert set(ran) == {"score_cross", "score_strips"}, ran
    assert all(int(g[:, 1].max()) == 0 for g in got)
    assert int(got[1][3, 5]) > 512 and int(got[5][3, 3]) > 100             # hits past the first seam, with counts


def test_several_tiles_at_one_mib(ctx):
    """chunk_bytes = 1 MiB: 60 x 700 pairs at 28 result bytes are more than one tile; the same matrices as at the default
    budget."""
    rng = random.Random(60700)
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    queries = [rand_seq(rng, rng.randint(20, 300), b"ACGT") for _ in range(59)] + [rand_seq(rng, 800, b"ACGT")]
    targets = [rand_seq(rng, rng.randint(0, 200), b"ACGT") for _ in range(700)]
    q, t = W.seqset_from(queries), W.seqset_from(targets)
    whole = ctx.sw_stats_cross(q, t, sc)
    at_default = ctx.last_call()
    with ctx.options(chunk_bytes=MIB):
        got, ran = check_cross(ctx, queries, targets, sc, "1 MiB", oracle_sample=6)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, got))
    assert ran["score_cross"][0] > at_default["score_cross"][0] and "score_strips" in ran, (ran, at_default)


def test_empty_sets(ctx):
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    some, none = W.seqset_from([b"ACGT", b"AC"]), W.seqset_from([])
    assert all(g.shape == (2, 0) for g in ctx.sw_stats_cross(some, none, sc))
    assert all(g.shape == (0, 2) for g in ctx.sw_stats_cross(none, some, sc))


def named_pair(err):
    m = re.search(r"query (\d+), target (\d+):", str(err.value))
    assert err.value.code == S.E_UNKNOWN_PAIR and m, str(err.value)
    return int(m.group(1)), int(m.group(2))


def test_unknown_pair_is_named_by_query_and_target(ctx):
    """DNA_hybridization scores no pair with 'X'.  The pair named is the lowest one that meets it, through the CROSS form (a
    short query), through the strips on explicit pairs (the query of 600 letters) and for a target, and it is the pair
    sw_span_cross names on the same sets."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = random.Random(5)
    queries = [rand_seq(rng, n, b"ACGT") for n in (80, 600, 120, 90)]
    targets = [rand_seq(rng, 70, b"ACGT") for _ in range(20)]
    for bad_q, bad_t, want in ((2, None, (2, 0)),      # a short query (the CROSS form): its first target
                               (1, None, (1, 0)),      # a long one (the strips on explicit pairs)
                               (None, 11, (0, 11)),    # a target: the first query meets it first
                               (3, 11, (0, 11))):
        qs, ts = list(queries), list(targets)
        if bad_q is not None:
            qs[bad_q] = qs[bad_q][:30] + b"X" + qs[bad_q][31:]
        if bad_t is not None:
            ts[bad_t] = ts[bad_t][:5] + b"X" + ts[bad_t][6:]
        q, t = W.seqset_from(qs), W.seqset_from(ts)
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_stats_cross(q, t, hyb)
        with pytest.raises(S.SeqAlignError) as ref:
            ctx.sw_span_cross(q, t, hyb)
        assert named_pair(err) == named_pair(ref) == want, (str(err.value), str(ref.value))
    check_cross(ctx, queries, targets, hyb, "after the failures")


def test_unknown_pair_across_tiles(ctx):
    """test_gpu_sw_span_cross.py's sets: chunk_bytes = 1 MiB makes two target ranges.  X in query 8 fails (8, 0) in the first,
    X in target 2 916 fails (3, 2 916) in the second: the lower pair, found in the later tile, is the one named -- as without
    tiles.  (Every sequence is far below SEQALIGN_SW_STATS_MAX_LEN.)"""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = W.Rng(75)
    dna = lambda n: bytes(b"ACGT"[i] for i in rng.below(4, n))
    queries = [b"", b"", b""] + [dna(40 + 13 * i) for i in range(12)]
    queries[8] = queries[8][:3] + b"X" + queries[8][4:]
    filler = W.random_set(3000, 76, 150, 250, b"ACGT")
    targets = [dna(30 + 7 * j) for j in range(16)] + [filler.seq(j) for j in range(3000)]
    targets[2916] = targets[2916][:100] + b"X" + targets[2916][101:]
    q, t = W.seqset_from(queries), W.seqset_from(targets)
    with pytest.raises(S.SeqAlignError) as err_one:
        ctx.sw_stats_cross(q, t, hyb)
    with ctx.options(chunk_bytes=MIB):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_stats_cross(q, t, hyb)
        assert ctx.last_call()["score_cross"][0] >= 2
    assert named_pair(err) == named_pair(err_one) == (3, 2916)
