"""GPU tier: SW statistics matrices -- seqalign_sw_stats_cross (sa_batch_score_cross.hip, the CROSS form of sa_sw_stats.hip).

The seven [n_queries][n_targets] matrices must be what sw_stats returns on the explicit Q x T batch (pos_a / len_a in the query),
which tests/test_gpu_sw_stats.py holds to the oracle; the scores and spans are checked against the oracle here too."""
import random

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
