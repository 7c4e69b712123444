"""GPU tier: statistics matrices -- seqalign_nw_stats_cross (sa_batch_score_cross.hip, the CROSS form of sa_nw_stats.hip).

The three matrices equal nw_stats on the explicit Q x T batch (workloads.cross_batch), which test_gpu_nw_stats.py holds to the
oracle; a sample of the pairs is checked against the oracle here as well."""
import random
import re

import numpy as np
import pytest

import orclib as O
import seqalign_amd as S
import spanlib as SP
import statlib as ST
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def sets(seed, q_lens, n_targets, t_max):
    """Queries of the given lengths; ragged targets, every third one an indel relative of a stretch of some query."""
    rng = random.Random(seed)
    queries = [rand_seq(rng, n) for n in q_lens]
    targets = []
    for t in range(n_targets):
        if t % 3 == 0:
            q = queries[t % len(queries)]
            at = rng.randrange(max(1, len(q) - 100))
            targets.append(SP.indel_relative(rng, q[at:at + rng.randint(20, t_max)], b"ACGT")[:t_max])
        else:
            targets.append(rand_seq(rng, rng.randint(0, t_max)))
    return W.seqset_from(queries), W.seqset_from(targets)


def assert_equals_batch(ctx, q, t, sc, tag):
    explicit = ctx.nw_stats(W.cross_batch(q, t), sc)
    got = ctx.nw_stats_cross(q, t, sc)
    ran = ctx.last_call()
    for name, x, y in zip(("score", "matches", "mismatches"), got, explicit):
        assert x.shape == (q.n_seqs, t.n_seqs) and np.array_equal(x.ravel(), y), (tag, name)
    return got, ran


@pytest.mark.parametrize("init4", [[1, -2, -4, -1], [3, -1, -1, 0]], ids=["dna", "ext0"])
def test_matrices_equal_the_explicit_batch(ctx, init4):
    """Query lengths on both sides of 512 -- the CROSS form up to it, the strips on explicit pairs beyond -- every class of the
    ladder among the short ones, ragged targets with empty ones."""
    sc = S.make_scoring({"init": init4 + [0] * 6})
    q, t = sets(515 + init4[0], (100, 512, 513, 1100, 0, 64, 65, 200, 300, 330, 400), 37, 160)
    (score, m, mm), ran = assert_equals_batch(ctx, q, t, sc, str(init4))
    assert set(ran) == {"score_cross", "score_strips"} and ran["score_cross"] == (6, 9 * 37), ran   # six classes of the ladder
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    rng = random.Random(1)
    for _ in range(40):
        i, j = rng.randrange(q.n_seqs), rng.randrange(t.n_seqs)
        assert (int(score[i, j]), int(m[i, j]), int(mm[i, j])) == ST.want_one(osc, q.seq(i), t.seq(j)), (i, j)


def test_tiles_cut_by_a_small_budget(ctx):
    """1 MiB of chunk budget: the targets' results no longer fit one tile row of queries, so the matrix is cut into several
    tiles, and the long queries' pairs into several chunks."""
    sc = S.make_scoring({"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]})
    q, t = sets(99, [100, 512, 513, 1100] + [150] * 60, 3000, 60)
    explicit = ctx.nw_stats(W.cross_batch(q, t), sc)
    got = ctx.nw_stats_cross(q, t, sc)
    at_default = ctx.last_call()
    with ctx.options(chunk_bytes=MIB):
        cut = ctx.nw_stats_cross(q, t, sc)
        at_mib = ctx.last_call()
    for x, y, z in zip(got, cut, explicit):
        assert np.array_equal(x, y) and np.array_equal(x.ravel(), z)
    assert at_mib["score_cross"][0] > at_default["score_cross"][0], (at_mib, at_default)
    assert at_mib["score_cross"][1] == at_default["score_cross"][1] == 62 * 3000


def test_unknown_pair_is_named_by_query_and_target(ctx):
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = random.Random(5)
    queries = [rand_seq(rng, n) for n in (80, 600, 120, 90)]
    targets = [rand_seq(rng, 70) for _ in range(20)]
    for bad_q, bad_t, named in ((2, None, "query 2, target 0:"),      # a short query (the CROSS form): its first target
                                (1, None, "query 1, target 0:"),      # a long one (the strips on explicit pairs)
                                (None, 11, "query 0, target 11:"),    # a target: the first query meets it first
                                (3, 11, "query 0, target 11:")):
        qs, ts = list(queries), list(targets)
        if bad_q is not None:
            qs[bad_q] = qs[bad_q][:30] + b"X" + qs[bad_q][31:]
        if bad_t is not None:
            ts[bad_t] = ts[bad_t][:5] + b"X" + ts[bad_t][6:]
        with pytest.raises(S.SeqAlignError) as err:
            ctx.nw_stats_cross(W.seqset_from(qs), W.seqset_from(ts), hyb)
        with pytest.raises(S.SeqAlignError) as ref:
            ctx.nw_score_cross(W.seqset_from(qs), W.seqset_from(ts), hyb)
        assert err.value.code == ref.value.code == S.E_UNKNOWN_PAIR
        assert named in str(err.value) and named in str(ref.value), (str(err.value), str(ref.value))
    got, _ = assert_equals_batch(ctx, W.seqset_from(queries), W.seqset_from(targets), hyb, "after the failures")


def test_unknown_pair_across_tiles(ctx):
    """test_gpu_sw_span_cross.py's sets: chunk_bytes = 1 MiB makes two target ranges.  X in query 8 fails (8, 0) in the first,
    X in target 2 916 fails (3, 2 916) in the second: the lower pair, found in the later tile, is the one named -- as without
    tiles."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = W.Rng(75)
    dna = lambda n: bytes(b"ACGT"[i] for i in rng.below(4, n))
    queries = [b"", b"", b""] + [dna(40 + 13 * i) for i in range(12)]
    queries[8] = queries[8][:3] + b"X" + queries[8][4:]
    filler = W.random_set(3000, 76, 150, 250, b"ACGT")
    targets = [dna(30 + 7 * j) for j in range(16)] + [filler.seq(j) for j in range(3000)]
    targets[2916] = targets[2916][:100] + b"X" + targets[2916][101:]
    q, t = W.seqset_from(queries), W.seqset_from(targets)

    def named_pair(err):
        m = re.search(r"query (\d+), target (\d+):", str(err.value))
        assert err.value.code == S.E_UNKNOWN_PAIR and m, str(err.value)
        return int(m.group(1)), int(m.group(2))

    with pytest.raises(S.SeqAlignError) as err_one:
        ctx.nw_stats_cross(q, t, hyb)
    with ctx.options(chunk_bytes=MIB):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.nw_stats_cross(q, t, hyb)
        assert ctx.last_call()["score_cross"][0] >= 2
    assert named_pair(err) == named_pair(err_one) == (3, 2916)
