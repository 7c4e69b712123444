"""GPU tier: top-k score search -- seqalign_nw_score_search / seqalign_sw_score_search (sa_score_select.hip on the tiles of
sa_batch_score_cross.hip).

The contract: for query q, the targets t with score[q][t] >= min_score, where score is the cross call's on the same sets,
ordered by score descending then target ascending, the first min(k, count) of them with the cross call's end_a / end_b.
Checked against np.lexsort over the cross call's matrices, against the oracle, across tiles and tie groups, at a size whose
dense matrix is never built, on failing pairs, empty sets and several contexts.
"""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

DNA, PROTEIN = b"ACGT", bytes(W.AMINO20)
INT32_MIN = -2**31


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def rand_seq(rng, n, alpha):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


def cross(ctx, q, t, sc, is_sw, **kw):
    """(score, end_a, end_b) matrices of the cross call; NW: zero ends."""
    if is_sw:
        return ctx.sw_score_cross(q, t, sc, **kw)
    s = ctx.nw_score_cross(q, t, sc, **kw)
    return s, np.zeros(s.shape, np.uint32), np.zeros(s.shape, np.uint32)


def search(ctx, q, t, sc, is_sw, k, min_score, **kw):
    return (ctx.sw_score_search if is_sw else ctx.nw_score_search)(q, t, sc, k, min_score=min_score, **kw)


def top_k(score, end_a, end_b, k, min_score):
    """The contract on dense matrices: per row, (targets, scores, end_a, end_b) by np.lexsort."""
    out = []
    for row, ea, eb in zip(score, end_a, end_b):
        idx = np.nonzero(row.astype(np.int64) >= min_score)[0]
        order = idx[np.lexsort((idx, -row[idx].astype(np.int64)))][:k]
        out.append((order, row[order], ea[order], eb[order]))
    return out


def assert_hits(got, want, tag=""):
    n_hits, hits = got
    assert n_hits.shape == (len(want),) and hits.shape[0] == len(want)
    for q, (tg, sc, ea, eb) in enumerate(want):
        n = int(n_hits[q])
        assert n == len(tg), (tag, q, n, len(tg))
        h = hits[q, :n]
        assert np.array_equal(h["target"], tg), (tag, q, h["target"][:8], tg[:8])
        assert np.array_equal(h["score"], sc), (tag, q)
        assert np.array_equal(h["end_a"], ea) and np.array_equal(h["end_b"], eb), (tag, q)


def assert_same(a, b, tag=""):
    """Two search results, slot for slot up to n_hits."""
    assert np.array_equal(a[0], b[0]), tag
    for q in range(a[0].shape[0]):
        n = int(a[0][q])
        assert np.array_equal(a[1][q, :n], b[1][q, :n]), (tag, q)


# ---------------------------------------------------------------- 1. the cross call plus a host sort --
@pytest.fixture(scope="module")
def proteins():
    """~300 ragged proteins of 50-600 and three of 1 100-1 500 (the strips path), against 1 200 of 50-600."""
    q = W.random_set(300, 131, 50, 600, PROTEIN)
    rng = W.Rng(132)
    long_q = [rand_seq(rng, n, PROTEIN) for n in (1100, 1320, 1500)]
    qs = [q.seq(i) for i in range(120)] + long_q[:2] + [q.seq(i) for i in range(120, 300)] + long_q[2:]
    return W.seqset_from(qs), W.random_set(1200, 133, 50, 600, PROTEIN)


@pytest.mark.parametrize("k", [1, 7, 64, 1024])
def test_sw_proteins_equal_cross_plus_sort(ctx, proteins, k):
    q, t = proteins
    sc = S.make_scoring({"preset": "BLOSUM62"})
    want = top_k(*cross(ctx, q, t, sc, 1), k, 1)
    got = search(ctx, q, t, sc, 1, k, 1)
    calls = ctx.last_call()
    assert {"score_cross", "score_select", "score_strips"} <= set(calls), calls
    assert_hits(got, want, f"k={k}")


@pytest.mark.parametrize("min_score", [INT32_MIN, 40])
@pytest.mark.parametrize("k", [1, 7, 64, 1024])
def test_nw_dna_equal_cross_plus_sort(ctx, min_score, k):
    """NW scores of random reads are negative: INT32_MIN keeps every target.  300 targets are copies of queries (score = length,
    60 or more), so a positive cut keeps some of them and leaves the other queries none."""
    q = W.random_set(200, 141, 60, 200, DNA)
    rand_t = W.random_set(1500, 142, 60, 200, DNA)
    spots = set(np.random.default_rng(143).choice(1500, 300, replace=False).tolist())
    t = W.seqset_from([q.seq(j % 150) if j in spots else rand_t.seq(j) for j in range(1500)])
    sc = S.make_scoring({"preset": "default"})
    s = cross(ctx, q, t, sc, 0)
    if min_score > 0:
        passing = (s[0] >= min_score).sum(axis=1)
        assert passing.max() > 1 and (passing == 0).any()
    assert_hits(search(ctx, q, t, sc, 0, k, min_score), top_k(*s, k, min_score), f"k={k} min={min_score}")


@pytest.mark.parametrize("is_sw", [0, 1])
def test_k_over_n_targets(ctx, is_sw):
    """k > n_targets: every passing target, in order; SW with min_score 0 keeps the score-0 targets."""
    q, t = W.random_set(40, 151, 0, 90, DNA), W.random_set(30, 152, 0, 90, DNA)
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]} if is_sw else {"preset": "default"})
    for min_score in ((0, 1, 9) if is_sw else (INT32_MIN, -20)):
        want = top_k(*cross(ctx, q, t, sc, is_sw), 100, min_score)
        assert_hits(search(ctx, q, t, sc, is_sw, 100, min_score), want, f"min={min_score}")
    if is_sw:
        n_hits, _ = search(ctx, q, t, sc, 1, 100, 0)
        assert (n_hits == 30).all()


# ---------------------------------------------------------------- 2. tiles and ties --
@pytest.mark.parametrize("is_sw", [0, 1])
def test_ties_across_tiles(ctx, is_sw):
    """600 distinct targets, each 5x at scattered indices: equal scores everywhere, so k cuts inside tie groups.  Under
    chunk_bytes = 1 MiB the targets take two ranges and the queries several: the result equals the one-tile run and the
    lexsort of the cross call."""
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]} if is_sw else {"preset": "default"})
    distinct = W.random_set(600, 161, 150, 250, DNA)
    perm = np.random.default_rng(162).permutation(3000)
    t = W.seqset_from([distinct.seq(int(perm[j]) % 600) for j in range(3000)])
    q = W.random_set(100, 163, 20, 64, DNA)
    min_score = 1 if is_sw else INT32_MIN
    dense = cross(ctx, q, t, sc, is_sw)
    for k in (7, 64):
        want = top_k(*dense, k, min_score)
        one = search(ctx, q, t, sc, is_sw, k, min_score)
        assert ctx.last_call()["score_select"][0] == 1
        with ctx.options(chunk_bytes=1 << 20):
            many = search(ctx, q, t, sc, is_sw, k, min_score)
            calls = ctx.last_call()
        assert calls["score_select"][0] >= 4 and calls["score_select"][0] == calls["score_cross"][0], calls
        assert_hits(one, want, f"one k={k}")
        assert_hits(many, want, f"many k={k}")
        assert_same(one, many)
        # the cut falls inside a tie group somewhere
        cut = [q_ for q_ in range(q.n_seqs) if int(one[0][q_]) == k and
               (dense[0][q_] == one[1][q_, k - 1]["score"]).sum() > (one[1][q_]["score"] == one[1][q_, k - 1]["score"]).sum()]
        assert cut, "no query's k-th hit splits a tie group"


# ---------------------------------------------------------------- 3. the oracle --
def oracle_scores(osc, q, t, is_sw):
    """Dense (score, end_a, end_b) from the oracle's matrices (test_gpu_score_cross.py's rule)."""
    shape = (q.n_seqs, t.n_seqs)
    s, ea, eb = np.zeros(shape, np.int32), np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
    for i in range(q.n_seqs):
        for j in range(t.n_seqs):
            a, b = q.seq(i), t.seq(j)
            rc, M, A, B = O.oracle_fill(osc, a, b, is_sw)
            assert rc == 0
            if not is_sw:
                s[i, j] = max(M[-1], A[-1], B[-1])
                continue
            Mr = np.asarray(M, np.int64).reshape(len(b) + 1, len(a) + 1)
            best = int(Mr.max())
            if best > 0:
                rows, cols = np.nonzero(Mr == best)
                x = np.lexsort((rows, cols))[0]
                s[i, j], ea[i, j], eb[i, j] = best, cols[x], rows[x]
    return s, ea, eb


@pytest.mark.parametrize("is_sw", [0, 1])
def test_vs_oracle(ctx, is_sw):
    """Small sets with lower case, wildcards and mutations under several of the reference's flag combinations."""
    for idx, flags in enumerate(list(itertools.product([0, 1], repeat=5))[::5]):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        sc = S.make_scoring(spec)
        osc = O.Scoring.from_buffer_copy(bytes(sc))
        rng = W.Rng(900 + idx)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        q = W.seqset_from([rand_seq(rng, n, alpha) for n in (0, 5, 70, 33)])
        t = W.seqset_from([rand_seq(rng, n, alpha) for n in (12, 0, 90, 1, 64, 65, 12, 40)])
        dense = oracle_scores(osc, q, t, is_sw)
        for k, min_score in ((3, 1 if is_sw else INT32_MIN), (8, 0 if is_sw else -10)):
            assert_hits(search(ctx, q, t, sc, is_sw, k, min_score), top_k(*dense, k, min_score), f"flags={flags} k={k}")


# ---------------------------------------------------------------- 4. planted hits, no dense matrix --
def test_planted_hits_in_two_million_targets(ctx):
    """SW, 16 DNA queries of 64 against 2 M random targets of 64 with exact copies of each query planted at known indices:
    they come first, in index order, with score 64 x match, ending at (64, 64).  Nothing dense is built."""
    rng = np.random.default_rng(171)
    n_t, L = 2_000_000, 64
    alpha = np.frombuffer(DNA, np.uint8)
    queries = alpha[rng.integers(0, 4, (16, L))]
    targets = alpha[rng.integers(0, 4, (n_t, L))]
    planted = {}
    spots = rng.choice(n_t, 16 * 4, replace=False).reshape(16, 4)
    for qi in range(16):
        idx = np.sort(spots[qi][: 1 + qi % 4])
        targets[idx] = queries[qi]
        planted[qi] = idx
    def as_set(rows):
        n = rows.shape[0]
        return W.SeqSet(np.concatenate([rows.reshape(-1), np.zeros(1, np.uint8)]),
                        np.arange(n, dtype=np.uint64) * np.uint64(L), np.full(n, L, np.uint32))
    q, t = as_set(queries), as_set(targets)
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    n_hits, hits = ctx.sw_score_search(q, t, sc, 6)
    calls = ctx.last_call()
    assert set(calls) == {"score_cross", "score_select"}, calls
    for qi in range(16):
        idx = planted[qi]
        assert int(n_hits[qi]) == 6
        h = hits[qi]
        assert np.array_equal(h["target"][: len(idx)], idx), (qi, h["target"], idx)
        assert (h["score"][: len(idx)] == 128).all() and (h["end_a"][: len(idx)] == 64).all() and \
            (h["end_b"][: len(idx)] == 64).all()
        rest = h["score"][len(idx):]
        assert (rest < 128).all() and (np.diff(h["score"].astype(np.int64)) <= 0).all()


# ---------------------------------------------------------------- 5. errors and edges --
def named_pair(err):
    m = re.search(r"query (\d+), target (\d+):", str(err.value))
    assert err.value.code == S.E_UNKNOWN_PAIR and m, str(err.value)
    return int(m.group(1)), int(m.group(2))


def plant_x(seq, at):
    return seq[:at] + b"X" + seq[at + 1:]


@pytest.mark.parametrize("is_sw", [0, 1])
@pytest.mark.parametrize("tiles", [False, True])
def test_unknown_pair_names_what_the_cross_call_names(ctx, is_sw, tiles):
    """DNA_hybridization scores no pair with 'X'.  In one tile, and across two target ranges (chunk_bytes = 1 MiB, where
    the lower failing pair is found in the later tile), the search names the cross call's pair -- and so does _multi."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = W.Rng(181 + is_sw)
    queries = [b"", b"", b""] + [rand_seq(rng, 40 + 13 * i, DNA) for i in range(12)]
    queries[8] = plant_x(queries[8], 3)
    targets = [rand_seq(rng, 30 + 7 * j, DNA) for j in range(16)]
    if tiles:
        filler = W.random_set(3000, 183, 150, 250, DNA)
        targets += [filler.seq(j) for j in range(3000)]
        targets[2916] = plant_x(targets[2916], 100)
    else:
        targets[9] = plant_x(targets[9], 10)
    q, t = W.seqset_from(queries), W.seqset_from(targets)
    cross_call = ctx.sw_score_cross if is_sw else ctx.nw_score_cross
    opts = {"chunk_bytes": 1 << 20} if tiles else {}
    with ctx.options(**opts):
        with pytest.raises(S.SeqAlignError) as err_c:
            cross_call(q, t, hyb)
        with pytest.raises(S.SeqAlignError) as err_s:
            search(ctx, q, t, hyb, is_sw, 5, 1 if is_sw else INT32_MIN)
        if tiles:
            assert ctx.last_call()["score_select"][0] >= 2
    assert named_pair(err_s) == named_pair(err_c) == ((3, 2916) if tiles else (3, 9))
    assert str(err_s.value).split("] ", 1)[1] == str(err_c.value).split("] ", 1)[1]   # seqalign_last_error's text
    with S.Context(0) as peer:
        with pytest.raises(S.SeqAlignError) as err:
            search(ctx, W.seqset_from([b""] * 4 + queries), t, hyb, is_sw, 5, 0, peers=[peer])
    assert named_pair(err) == (named_pair(err_c)[0] + 4, named_pair(err_c)[1])
    ok = search(ctx, W.seqset_from(queries[9:11]), W.seqset_from(targets[:3]), S.make_scoring({"preset": "default"}),
                is_sw, 2, INT32_MIN)
    assert list(ok[0]) == [2, 2]                                  # the context still works


def test_empty_sets(ctx):
    sc = S.make_scoring({"preset": "default"})
    none, some = W.seqset_from([]), W.seqset_from([b"ACGT", b"GG"])
    n_hits, hits = ctx.nw_score_search(none, some, sc, 3)
    assert n_hits.shape == (0,) and hits.shape == (0, 3)
    n_hits = np.full(2, 7, np.uint32)
    hits = np.zeros((2, 3), S.SEARCH_HIT)
    dq, dt = S.seqset_desc(some), S.seqset_desc(none)
    assert S.lib().seqalign_sw_score_search(ctx._h, C.byref(dq), C.byref(dt), C.byref(sc), C.c_uint32(3), C.c_int32(1),
                                            S._ptr(hits), S._ptr(n_hits)) == 0
    assert list(n_hits) == [0, 0]                                 # no targets: every count written
    assert ctx.last_call() == {}
    with S.Context(0) as peer:
        n_hits, _ = ctx.sw_score_search(some, none, sc, 3, peers=[peer])
        assert list(n_hits) == [0, 0]
        n_hits, _ = ctx.sw_score_search(some, some, sc, 3, min_score=10**6, peers=[peer])
        assert list(n_hits) == [0, 0]                             # nothing passes the cut


# ---------------------------------------------------------------- 6. several contexts --
@pytest.mark.parametrize("is_sw", [0, 1])
def test_multi_context_equals_single(ctx, is_sw):
    rng = W.Rng(191)
    q = W.seqset_from([rand_seq(rng, n, DNA) for n in rng.below(700, 60).tolist()] + [rand_seq(rng, 1400, DNA)])
    t = W.random_set(400, 192, 0, 300, DNA)
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]} if is_sw else {"preset": "default"})
    min_score = 1 if is_sw else INT32_MIN
    one = search(ctx, q, t, sc, is_sw, 16, min_score)
    with S.Context(0) as peer:
        two = search(ctx, q, t, sc, is_sw, 16, min_score, peers=[peer])
    assert_same(one, two)
    assert_hits(one, top_k(*cross(ctx, q, t, sc, is_sw), 16, min_score))


# ---------------------------------------------------------------- 7. launches --
def test_launches(ctx):
    """score_cross per row class, one score_select per tile over its rows; nothing else (no strips for short queries)."""
    sc = S.make_scoring({"preset": "default"})
    rng = W.Rng(201)
    q = W.seqset_from([rand_seq(rng, n, DNA) for n in (10, 100, 1000, 1024, 300)])
    t = W.random_set(50, 202, 0, 200, DNA)
    ctx.nw_score_search(q, t, sc, 4)
    calls = ctx.last_call()
    assert set(calls) == {"score_cross", "score_select"}, calls
    assert calls["score_cross"] == (4, 5 * 50) and calls["score_select"] == (1, 5), calls


# ---------------------------------------------------------------- 8. all 32 key bits --
# Every search above has rows whose scores span fewer than 2 048 values, or keys so small that each radix pass has one or two
# populated bins.  Under a scoring with large odd constants the three passes carry a prefix, a rank and a cut between them.
MAG_SPEC = {"init": [2**20 + 7, -3 * (2**16 + 1), -5 * (2**16 + 1), -33 * (2**16 + 1), 0, 0, 0, 0, 0, 0]}
MAG_K = (1, 7, 64, 1024)


def related(rng, s):
    """A relative of s: about one letter in eight substituted, one deleted."""
    out = bytearray(s)
    for i in rng.below(len(out), max(1, len(out) // 8)).tolist():
        out[i] = DNA[int(rng.below(4, 1)[0])]
    del out[int(rng.below(len(out), 1)[0])]
    return bytes(out)


@pytest.fixture(scope="module")
def magnitude_sets():
    """64 queries of 20-60 against 3 000 targets of 20-60: 600 distinct ones, each five times at scattered indices; every sixth
    distinct target is a relative of a query."""
    rng = W.Rng(211)
    queries = [rand_seq(rng, int(n), DNA) for n in (20 + rng.below(41, 64)).tolist()]
    distinct = [rand_seq(rng, int(n), DNA) for n in (20 + rng.below(41, 600)).tolist()]
    for d in range(0, 600, 6):
        distinct[d] = related(rng, queries[(d // 6) % 64])
    perm = np.random.default_rng(212).permutation(3000)
    return W.seqset_from(queries), W.seqset_from([distinct[int(perm[j]) % 600] for j in range(3000)])


def splits_a_tie_group(dense, got, k):
    """Queries whose k-th hit has equals among the targets left out."""
    n_hits, hits = got
    return [q for q in range(len(n_hits)) if int(n_hits[q]) == k and
            (dense[0][q] == hits[q, k - 1]["score"]).sum() > (hits[q]["score"] == hits[q, k - 1]["score"]).sum()]


@pytest.mark.parametrize("is_sw", [0, 1])
def test_select_with_all_key_bits_in_play(ctx, magnitude_sets, is_sw):
    """Rows whose passing scores span more than 2^11 and more than 2^22 values (three radix passes with many populated bins),
    NW rows of both signs, and for k = 1, 7, 64 and 1 024 a cut inside a tie group: one tile, and query ranges under
    chunk_bytes = 1 MiB, equal to each other and to the lexsort of the cross call."""
    q, t = magnitude_sets
    sc = S.make_scoring(MAG_SPEC)
    floor = 1 if is_sw else INT32_MIN
    dense = cross(ctx, q, t, sc, is_sw)
    s = dense[0].astype(np.int64)
    spans = [int(r[r >= floor].max() - r[r >= floor].min()) for r in s if (r >= floor).sum() > 1024]
    assert len(spans) == q.n_seqs and max(spans) > 2**22 and min(spans) > 2**11, (len(spans), min(spans), max(spans))
    varying = int(np.bitwise_or.reduce((s ^ s[0, 0]).ravel())) & 0xFFFFFFFF
    # every key bit up to the highest one that differs takes both values: all 32 under NW (the first pass starts at bit 32),
    # the 26 that 60 matches reach under SW
    assert varying == (1 << varying.bit_length()) - 1 and varying.bit_length() >= (26 if is_sw else 32), hex(varying)
    if not is_sw:
        assert any((r > 0).any() and (r < 0).any() for r in s)
    for k in MAG_K:
        want = top_k(*dense, k, floor)
        one = search(ctx, q, t, sc, is_sw, k, floor)
        assert ctx.last_call()["score_select"][0] == 1
        with ctx.options(chunk_bytes=1 << 20):
            many = search(ctx, q, t, sc, is_sw, k, floor)
            calls = ctx.last_call()
        # (SW's 12 bytes per result cut the queries into ranges; NW's 4 leave this set in one tile: the 15 000 targets below)
        assert calls["score_select"][0] >= (2 if is_sw else 1) and calls["score_select"][0] == calls["score_cross"][0], calls
        assert_hits(one, want, f"one k={k}")
        assert_hits(many, want, f"many k={k}")
        assert_same(one, many)
        assert splits_a_tie_group(dense, one, k), f"k={k}: no query's k-th hit splits a tie group"


@pytest.mark.parametrize("is_sw", [0, 1])
def test_select_min_score_edges_at_large_scores(ctx, magnitude_sets, is_sw):
    """min_score at INT32_MIN, at INT32_MAX (nothing passes), at exactly a row's k-th score and one above it."""
    q, t = magnitude_sets
    sc = S.make_scoring(MAG_SPEC)
    dense = cross(ctx, q, t, sc, is_sw)
    for k in (7, 64):
        kth = int(top_k(*dense, k, 1 if is_sw else INT32_MIN)[5][1][k - 1])
        for min_score in (INT32_MIN, 2**31 - 1, kth, kth + 1):
            want = top_k(*dense, k, min_score)
            one = search(ctx, q, t, sc, is_sw, k, min_score)
            with ctx.options(chunk_bytes=1 << 20):
                many = search(ctx, q, t, sc, is_sw, k, min_score)
            assert_hits(one, want, f"k={k} min={min_score}")
            assert_same(one, many, f"k={k} min={min_score}")
        assert int(search(ctx, q, t, sc, is_sw, k, 2**31 - 1)[0].sum()) == 0
        assert int(search(ctx, q, t, sc, is_sw, k, kth)[0][5]) == k > int(search(ctx, q, t, sc, is_sw, k, kth + 1)[0][5])


@pytest.mark.parametrize("is_sw", [0, 1])
def test_select_carries_large_keys_across_target_ranges(ctx, magnitude_sets, is_sw):
    """The same targets five times over (15 000): under chunk_bytes = 1 MiB they take several ranges, so the running lists --
    keys with all bits in play -- go through the select again with every later range."""
    q, t3 = magnitude_sets
    t = W.seqset_from([t3.seq(j % 3000) for j in range(15000)])
    sc = S.make_scoring(MAG_SPEC)
    floor = 1 if is_sw else INT32_MIN
    dense = cross(ctx, q, t, sc, is_sw)
    for k in (7, 1024):
        with ctx.options(chunk_bytes=1 << 20):
            many = search(ctx, q, t, sc, is_sw, k, floor)
            calls = ctx.last_call()
        assert calls["score_select"][1] >= 2 * q.n_seqs, calls          # rows selected: every query once per target range
        assert_hits(many, top_k(*dense, k, floor), f"k={k}")
        assert_same(many, search(ctx, q, t, sc, is_sw, k, floor))
