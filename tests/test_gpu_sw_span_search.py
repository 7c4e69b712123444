"""GPU tier: top-k search with spans -- seqalign_sw_span_search (seqalign_sw_score_search's selection, then the span sweep on
the selected hits' prefix pairs; sa_batch_score_cross.hip).

The contract: n_hits and every slot's target and score are sw_score_search's on the same arguments; pos / len are
sw_span_cross's at [q, target]; pos + len is the score search's end; a hit of score 0 has five zeros.  Checked against the
top k taken on the host from sw_span_cross's matrices, against sw_score_search, over prefixes that run the one-wave kernel
and the strips, across tiles and tie groups, on failing pairs and over several contexts.
"""
import re

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

DNA = b"ACGT"
DNA_SW = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}
INT32_MIN = -2**31
FIELDS = ("score", "pos_a", "pos_b", "len_a", "len_b")


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def rand_seq(rng, n, alpha=DNA):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


def relative(rng, s, alpha=DNA):
    """About one letter in ten substituted, deleted or preceded by an inserted one."""
    out = bytearray()
    for ch in s:
        r = int(rng.below(30, 1)[0])
        if r == 0:
            continue
        if r == 1:
            out.append(alpha[int(rng.below(len(alpha), 1)[0])])
        out.append(alpha[int(rng.below(len(alpha), 1)[0])] if r == 2 else ch)
    return bytes(out)


def top_k(dense, k, min_score):
    """The contract on sw_span_cross's matrices: per row the targets by np.lexsort, and their five fields."""
    out = []
    for q, row in enumerate(dense[0]):
        idx = np.nonzero(row.astype(np.int64) >= min_score)[0]
        order = idx[np.lexsort((idx, -row[idx].astype(np.int64)))][:k]
        out.append((order, [m[q][order] for m in dense]))
    return out


def assert_hits(got, want, tag=""):
    n_hits, hits = got
    assert n_hits.shape == (len(want),) and hits.shape[0] == len(want) and hits.dtype == S.SPAN_HIT
    for q, (tg, fields) in enumerate(want):
        n = int(n_hits[q])
        assert n == len(tg), (tag, q, n, len(tg))
        h = hits[q, :n]
        assert np.array_equal(h["target"], tg), (tag, q, h["target"][:8], tg[:8])
        for name, w in zip(FIELDS, fields):
            assert np.array_equal(h[name], w), (tag, q, name, h[name][:8], w[:8])


def assert_is_the_score_search(got, score_got, tag=""):
    """n_hits, targets and scores are sw_score_search's; pos + len its ends; a hit of score 0 has five zeros."""
    assert np.array_equal(got[0], score_got[0]), tag
    for q in range(got[0].shape[0]):
        n = int(got[0][q])
        h, s = got[1][q, :n], score_got[1][q, :n]
        assert np.array_equal(h["target"], s["target"]) and np.array_equal(h["score"], s["score"]), (tag, q)
        assert np.array_equal(h["pos_a"] + h["len_a"], s["end_a"]) and np.array_equal(h["pos_b"] + h["len_b"], s["end_b"]), (tag, q)
        zero = h[h["score"] == 0]
        assert not any(zero[name].any() for name in FIELDS), (tag, q)


def assert_same(a, b, tag=""):
    assert np.array_equal(a[0], b[0]), tag
    for q in range(a[0].shape[0]):
        n = int(a[0][q])
        assert np.array_equal(a[1][q, :n], b[1][q, :n]), (tag, q)


# ---------------------------------------------------------------- 1. the span matrices plus a host sort --
@pytest.fixture(scope="module")
def reads():
    """48 queries of 0 .. 300 (two empty, two of one letter only) against 80 targets of 0 .. 300, a third of them relatives of
    stretches of queries; 'W' pairs with nothing, so some scores are 0."""
    rng = W.Rng(301)
    queries = [rand_seq(rng, int(n)) for n in rng.below(301, 44).tolist()] + [b"", b"W" * 30, b"", b"W"]
    targets = []
    for j in range(80):
        src = queries[j % 44]
        if j % 3 == 0 and len(src) >= 40:
            at = int(rng.below(len(src) - 30, 1)[0])
            targets.append(rand_seq(rng, j % 7) + relative(rng, src[at:at + 120]) + rand_seq(rng, j % 11))
        elif j % 20 == 7:
            targets.append(b"W" * (j % 3))
        else:
            targets.append(rand_seq(rng, int(rng.below(301, 1)[0])))
    return W.seqset_from(queries), W.seqset_from(targets)


@pytest.fixture(scope="module")
def reads_dense(ctx, reads):
    return ctx.sw_span_cross(*reads, S.make_scoring(DNA_SW))


@pytest.mark.parametrize("min_score", [1, 60, 0, INT32_MIN])
@pytest.mark.parametrize("k", [1, 7, 64, 83])
def test_equals_span_cross_plus_sort(ctx, reads, reads_dense, k, min_score):
    """k = 1, 7, 64 and n_targets + 3; min_score 1, 60 (cuts most lists short), and 0 and INT32_MIN, which select the targets
    of score 0: those come back as five zeros."""
    q, t = reads
    sc = S.make_scoring(DNA_SW)
    got = ctx.sw_span_search(q, t, sc, k, min_score=min_score)
    assert_hits(got, top_k(reads_dense, k, min_score), (k, min_score))
    assert_is_the_score_search(got, ctx.sw_score_search(q, t, sc, k, min_score=min_score), (k, min_score))
    if min_score == 60:
        assert (got[0] < min(k, 80)).any() and (got[0] > 0).any()
    if min_score <= 0 and k > 7:
        assert sum(int((got[1][i, :int(got[0][i])]["score"] == 0).sum()) for i in range(q.n_seqs)) > 80
        assert (got[0] == min(k, 80)).all()


# ---------------------------------------------------------------- 2. prefixes on both kernels --
def test_long_queries_prefixes_run_rows_and_strips(ctx):
    """Queries of 600 and 1 100 columns (the first stage's one-wave kernel and strips) with relatives planted: of query 0 one
    that ends before column 512 -- its prefix pair runs the one-wave span kernel -- and one that ends past it; of query 1 one
    that ends past column 1 024 (three strips) and one before 512.  Query 0's hits are of both kinds."""
    rng = W.Rng(311)
    q0, q1, q2 = rand_seq(rng, 600), rand_seq(rng, 1100), rand_seq(rng, 90)
    targets = [rand_seq(rng, int(n)) for n in (40 + rng.below(200, 20)).tolist()]
    targets[3] = rand_seq(rng, 15) + relative(rng, q0[100:300]) + rand_seq(rng, 20)
    targets[8] = relative(rng, q0[440:590]) + rand_seq(rng, 9)
    targets[11] = rand_seq(rng, 30) + relative(rng, q1[880:1090])
    targets[14] = relative(rng, q1[200:400])
    targets[17] = relative(rng, q2)
    q, t = W.seqset_from([q0, q1, q2]), W.seqset_from(targets)
    sc = S.make_scoring(DNA_SW)
    dense = ctx.sw_span_cross(q, t, sc)
    for k in (2, 5):
        got = ctx.sw_span_search(q, t, sc, k)
        calls = ctx.last_call()
        assert {"score_cross", "score_select", "score_rows", "score_strips"} == set(calls), calls
        assert_hits(got, top_k(dense, k, 1), k)
        assert_is_the_score_search(got, ctx.sw_score_search(q, t, sc, k), k)
    n_hits, hits = got
    end_a = (hits["pos_a"] + hits["len_a"]).astype(np.int64)
    assert sorted(hits[0, :2]["target"].tolist()) == [3, 8] and sorted(hits[1, :2]["target"].tolist()) == [11, 14]
    assert sorted(end_a[0, :2].tolist())[0] < 512 < sorted(end_a[0, :2].tolist())[1]
    assert sorted(end_a[1, :2].tolist())[0] < 512 and sorted(end_a[1, :2].tolist())[1] > 1024
    assert (hits[:, :2]["len_a"] > 100).sum() >= 4 and (hits[:2, :2]["pos_a"] > 50).all()


# ---------------------------------------------------------------- 3. tiles and ties --
def test_ties_across_tiles(ctx):
    """600 distinct targets, each 5x at scattered indices: equal scores everywhere, so k cuts inside tie groups.  Under
    chunk_bytes = 1 MiB the targets take two ranges and the queries several: the result equals the one-tile run and the
    lexsort of the span matrices."""
    sc = S.make_scoring(DNA_SW)
    distinct = W.random_set(600, 161, 150, 250, DNA)
    perm = np.random.default_rng(162).permutation(3000)
    t = W.seqset_from([distinct.seq(int(perm[j]) % 600) for j in range(3000)])
    q = W.random_set(100, 163, 20, 64, DNA)
    dense = ctx.sw_span_cross(q, t, sc)
    for k in (7, 64):
        want = top_k(dense, k, 1)
        one = ctx.sw_span_search(q, t, sc, k)
        assert ctx.last_call()["score_select"][0] == 1
        with ctx.options(chunk_bytes=1 << 20):
            many = ctx.sw_span_search(q, t, sc, k)
            calls = ctx.last_call()
        assert calls["score_select"][0] >= 4 and calls["score_select"][0] == calls["score_cross"][0], calls
        assert calls["score_rows"][1] == int(many[0].sum())          # stage 2 swept the selected hits, and only them
        assert_hits(one, want, f"one k={k}")
        assert_hits(many, want, f"many k={k}")
        assert_same(one, many)
        cut = [i for i in range(q.n_seqs) if int(one[0][i]) == k and
               (dense[0][i] == one[1][i, k - 1]["score"]).sum() > (one[1][i]["score"] == one[1][i, k - 1]["score"]).sum()]
        assert cut, "no query's k-th hit splits a tie group"


# ---------------------------------------------------------------- 4. unknown pairs --
def named_pair(err):
    m = re.search(r"query (\d+), target (\d+):", str(err.value))
    assert err.value.code == S.E_UNKNOWN_PAIR and m, str(err.value)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("where", ["outside_the_best_k", "behind_the_end_cell"])
def test_unknown_character_fails_the_call(ctx, where):
    """DNA_hybridization scores no pair with 'X'.  k = 1 and every query has an exact copy among the targets, its best hit.
    An X in another target (a pair outside the best k), or behind the copy in the selected target itself (past the hit's end
    cell), fails the call as it fails sw_score_search: same code, same message; _multi names the pair in indices of the whole
    set."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = W.Rng(321)
    queries = [b""] + [rand_seq(rng, 50 + 9 * i) for i in range(6)]
    targets = [rand_seq(rng, 40 + 5 * j) for j in range(10)]
    for i in range(1, 7):
        targets[i] = queries[i]
    if where == "outside_the_best_k":
        targets[8] = targets[8][:20] + b"X" + targets[8][21:]
        want = (1, 8)
    else:
        targets[3] = queries[3] + b"ACX"
        want = (1, 3)
    q, t = W.seqset_from(queries), W.seqset_from(targets)
    with pytest.raises(S.SeqAlignError) as err_score:
        ctx.sw_score_search(q, t, hyb, 1)
    with pytest.raises(S.SeqAlignError) as err:
        ctx.sw_span_search(q, t, hyb, 1)
    assert named_pair(err) == named_pair(err_score) == want
    assert str(err.value).split("] ", 1)[1] == str(err_score.value).split("] ", 1)[1]   # seqalign_last_error's text
    with S.Context(0) as peer:
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_span_search(W.seqset_from([b""] * 4 + queries), t, hyb, 1, peers=[peer])
    assert named_pair(err) == (want[0] + 4, want[1])
    clean = W.seqset_from([x.replace(b"X", b"A") for x in targets])
    n_hits, hits = ctx.sw_span_search(q, clean, hyb, 1)              # the context still works; the copies are the best hits
    assert list(n_hits) == [0] + [1] * 6 and hits[1:, 0]["target"].tolist() == list(range(1, 7))
    assert hits[1:, 0]["pos_a"].tolist() == [0] * 6 and hits[1:, 0]["len_a"].tolist() == [len(x) for x in queries[1:]]


# ---------------------------------------------------------------- 5. edges, several contexts, launches --
def test_empty_sets(ctx):
    sc = S.make_scoring(DNA_SW)
    none, some = W.seqset_from([]), W.seqset_from([b"ACGT", b"GG"])
    n_hits, hits = ctx.sw_span_search(none, some, sc, 3)
    assert n_hits.shape == (0,) and hits.shape == (0, 3)
    n_hits, hits = ctx.sw_span_search(some, none, sc, 3)
    assert list(n_hits) == [0, 0] and ctx.last_call() == {}
    n_hits, hits = ctx.sw_span_search(some, some, sc, 3, min_score=10**6)
    assert list(n_hits) == [0, 0] and set(ctx.last_call()) == {"score_cross", "score_select"}   # no hit: no second stage


def test_multi_context_equals_single(ctx):
    rng = W.Rng(191)
    q = W.seqset_from([rand_seq(rng, n) for n in rng.below(700, 60).tolist()] + [rand_seq(rng, 1400)])
    t = W.random_set(400, 192, 0, 300, DNA)
    sc = S.make_scoring(DNA_SW)
    one = ctx.sw_span_search(q, t, sc, 16)
    with S.Context(0) as peer:
        two = ctx.sw_span_search(q, t, sc, 16, peers=[peer])
    assert_same(one, two)
    assert_hits(one, top_k(ctx.sw_span_cross(q, t, sc), 16, 1))


def test_launches(ctx, reads):
    """Stage 1 is the score search's launches; stage 2 sweeps one pair per hit above 0, through the one-wave span kernel."""
    q, t = reads
    sc = S.make_scoring(DNA_SW)
    n_hits, hits = ctx.sw_span_search(q, t, sc, 4)
    calls = ctx.last_call()
    ctx.sw_score_search(q, t, sc, 4)
    stage1 = ctx.last_call()
    assert set(calls) == {"score_cross", "score_select", "score_rows"}, calls
    assert {k: calls[k] for k in stage1} == stage1
    assert calls["score_rows"][1] == int(n_hits.sum())
