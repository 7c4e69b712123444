"""GPU tier: span matrices -- seqalign_sw_span_cross (sa_span.hip's cross form of the one-wave kernel, the span strips for
queries over 512 columns, sa_batch_score_cross.hip's tiles with 20 result bytes per pair).

The contract: the result of seqalign_sw_span_batch on the batch whose pair q * n_targets + t is (query q, target t)
(workloads.cross_batch), as five dense row-major matrices; score and pos + len are seqalign_sw_score_cross's.  Every case is
compared bit for bit with sw_span on that batch, small cells with the oracle's first hit as well.
"""
import itertools
import re

import numpy as np
import pytest

import maglib as G
import orclib as O
import seqalign_amd as S
import spanlib as SP
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

DNA = b"ACGT"
DNA_SW = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def rand_seq(rng, n, alpha):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


def relative(rng, s, alpha):
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


def explicit(ctx, q, t, sc):
    """sw_span on the materialised batch, as five [nq, nt] matrices."""
    return tuple(x.reshape(q.n_seqs, t.n_seqs) for x in ctx.sw_span(W.cross_batch(q, t), sc))


def assert_equal(got, want, tag=""):
    assert len(got) == len(want) == 5
    for name, g, w in zip(("score", "pos_a", "pos_b", "len_a", "len_b"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, name)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (tag, name, bad[:5].tolist())


def assert_ends(ctx, got, q, t, sc, tag=""):
    """score and pos + len are sw_score_cross's score and ends."""
    s, ea, eb = ctx.sw_score_cross(q, t, sc)
    assert np.array_equal(got[0], s), tag
    assert np.array_equal(got[1] + got[3], ea) and np.array_equal(got[2] + got[4], eb), tag


# ---------------------------------------------------------------- 1. every width --
# both sides of every columns-per-lane step of the span kernels (1 .. 6, 8), the one-wave limit (512) and the strips past it
QUERY_LENS = [0, 1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512, 513, 700, 1100]
TARGET_LENS = [0, 1, 50, 60, 90, 120, 150, 180, 210, 240, 270, 300]
WIDTH_SCORINGS = [("dna_sw", DNA_SW, DNA), ("open0", {"init": SP.TIE_SCORINGS["open0"] + [0] * 6}, b"AC"),
                  ("ext_pos", {"init": SP.TIE_SCORINGS["ext_pos"] + [0] * 6}, DNA)]


# target -> (query, first column) of the stretch of that query it is a relative of, as long as the target: of the 1 100-column
# query one past column 1 024 and one between 512 and 1 024, of the 700-column query one past 512
PLANTED = {4: (17, 1005), 5: (17, 520), 6: (16, 545), 8: (15, 300), 10: (14, 240), 7: (12, 200)}


def width_sets(seed, alpha):
    """Queries of QUERY_LENS; targets of TARGET_LENS, those of PLANTED relatives of a stretch of a query."""
    rng = W.Rng(seed)
    queries = [rand_seq(rng, n, alpha) for n in QUERY_LENS]
    targets = []
    for j, n in enumerate(TARGET_LENS):
        if j in PLANTED:
            i, at = PLANTED[j]
            targets.append(relative(rng, queries[i][at:at + n], alpha))
        else:
            targets.append(rand_seq(rng, n, alpha))
    return W.seqset_from(queries), W.seqset_from(targets)


@pytest.mark.parametrize("name,spec,alpha", WIDTH_SCORINGS, ids=[w[0] for w in WIDTH_SCORINGS])
def test_every_width_equals_the_pairwise_call(ctx, name, spec, alpha):
    sc = S.make_scoring(spec)
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    q, t = width_sets(5100 + len(name), alpha)
    got = ctx.sw_span_cross(q, t, sc)
    calls = ctx.last_call()
    # one score_cross launch per class of 1, 2, 3, 4, 5, 6 and 8 columns per lane, every short pair once; the three long
    # queries' pairs as one list through the span strips
    assert calls == {"score_cross": (7, 15 * 12), "score_strips": (1, 3 * 12)}, calls
    assert_equal(got, explicit(ctx, q, t, sc), name)
    assert_ends(ctx, got, q, t, sc, name)
    if name == "dna_sw":    # (over two letters, or with gaps that pay, other stretches score as much): the planted relatives are the hits
        for j, (i, at) in PLANTED.items():
            assert at <= int(got[1][i, j]) + int(got[3][i, j]) // 2 <= at + TARGET_LENS[j], (i, j)
            assert 2 * int(got[3][i, j]) > TARGET_LENS[j], (i, j)
        assert int(got[1][17, 4] + got[3][17, 4]) > 1024 and int(got[1][16, 6] + got[3][16, 6]) > 512 > int(got[1][16, 6]) - 100
    # cells of at most 64 x 64 against the oracle's first hit
    qi = [i for i, n in enumerate(QUERY_LENS) if n <= 64]
    tj = [j for j, n in enumerate(TARGET_LENS) if n <= 64]
    small = W.from_pairs([(q.seq(i), t.seq(j)) for i in qi for j in tj])
    assert [tuple(int(x[i, j]) for x in got) for i in qi for j in tj] == SP.want_spans(osc, small)


# ---------------------------------------------------------------- 2. ties --
@pytest.mark.parametrize("width", [200, 400])
@pytest.mark.parametrize("name", list(SP.TIE_SCORINGS))
def test_tie_dense_sets(ctx, name, width):
    """spanlib.tie_pairs as sets: all 40 seq_a against all 40 seq_b.  The diagonal holds the pairs themselves, of which the
    share tests/test_gpu_sw_span_dense.py counts changes its span when the predecessor priority is reversed."""
    sc = S.make_scoring({"init": SP.TIE_SCORINGS[name] + [0] * 6})
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    pairs = SP.tie_pairs(name, width)
    q, t = W.seqset_from([a for a, _ in pairs]), W.seqset_from([b for _, b in pairs])
    got = ctx.sw_span_cross(q, t, sc)
    assert set(ctx.last_call()) == {"score_cross"}
    assert_equal(got, explicit(ctx, q, t, sc), (name, width))
    both = [SP.walk_both(osc, a, b) for a, b in pairs]
    sensitive = sum(w != r for w, r in both)
    assert sensitive >= (len(pairs) // 2 if name == "ext_pos" else len(pairs) // 10), sensitive
    assert [tuple(int(x[p, p]) for x in got) for p in range(len(pairs))] == [w for w, _ in both]


# ---------------------------------------------------------------- 3. flags --
def test_all_flag_combinations(ctx):
    """The 32 combinations of the reference's five flags (the GENERAL sweep) on a 5 x 7 set, with lower case, wildcards and
    mutations: the pairwise call and the oracle's first hit."""
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        sc = S.make_scoring(spec)
        osc = O.Scoring.from_buffer_copy(bytes(sc))
        rng = W.Rng(800 + idx)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        q = W.seqset_from([rand_seq(rng, n, alpha) for n in (0, 5, 70, 33, 140)])
        t = W.seqset_from([rand_seq(rng, n, alpha) for n in (12, 0, 90, 1, 64, 65, 120)])
        got = ctx.sw_span_cross(q, t, sc)
        assert_equal(got, explicit(ctx, q, t, sc), flags)
        batch = W.cross_batch(q, t)
        assert [tuple(int(x.reshape(-1)[p]) for x in got) for p in range(batch.n_pairs)] == SP.want_spans(osc, batch), flags


# ---------------------------------------------------------------- 4. tiles --
def test_tiles_equal_one_tile(ctx):
    """chunk_bytes = 1 MiB: the targets (~600 KB) take two target ranges, the 20 result bytes per pair cut the queries into
    several ranges; the matrices equal the default budget's single tile.  Long queries take the strips in slices."""
    sc = S.make_scoring(DNA_SW)
    q, t = W.random_set(100, 51, 20, 64, DNA), W.random_set(3000, 52, 150, 250, DNA)
    one = ctx.sw_span_cross(q, t, sc)
    assert ctx.last_call() == {"score_cross": (1, 100 * 3000)}
    with ctx.options(chunk_bytes=1 << 20):
        many = ctx.sw_span_cross(q, t, sc)
        launches, waves = ctx.last_call()["score_cross"]
    assert launches >= 4 and launches % 2 == 0 and waves == 100 * 3000, (launches, waves)   # >= 2 query x 2 target ranges
    assert_equal(many, one)
    assert_ends(ctx, one, q, t, sc)
    rng = W.Rng(53)
    q2 = W.seqset_from([q.seq(0), rand_seq(rng, 1500, DNA), q.seq(1), rand_seq(rng, 600, DNA)])
    t2 = W.seqset_from([t.seq(j) for j in range(40)])
    one = ctx.sw_span_cross(q2, t2, sc)
    with ctx.options(chunk_bytes=1 << 20):
        many = ctx.sw_span_cross(q2, t2, sc)
    assert_equal(many, one)
    assert_equal(one, explicit(ctx, q2, t2, sc))


# ---------------------------------------------------------------- 5. unknown pairs --
def named_pair(err):
    m = re.search(r"query (\d+), target (\d+):", str(err.value))
    assert err.value.code == S.E_UNKNOWN_PAIR and m, str(err.value)
    return int(m.group(1)), int(m.group(2))


def pairwise_pair(ctx, q, t, sc):
    """(query, target) of the pair sw_span names on the materialised batch."""
    with pytest.raises(S.SeqAlignError) as err:
        ctx.sw_span(W.cross_batch(q, t), sc)
    m = re.search(r"pair (\d+):", str(err.value))
    assert err.value.code == S.E_UNKNOWN_PAIR and m, str(err.value)
    return divmod(int(m.group(1)), t.n_seqs)


def plant_x(seq, at):
    return seq[:at] + b"X" + seq[at + 1:]


@pytest.mark.parametrize("long_query", [False, True])
def test_unknown_pair_names_the_lowest_pair(ctx, long_query):
    """DNA_hybridization scores no pair with 'X'.  X in query 5 fails it against every non-empty target, X in target 9 every
    non-empty query: queries 0 .. 2 are empty, so the lowest failing pair is (3, 9) -- or (1, 0) when query 1 is a query of
    the strips path with an X.  The pair named is the one sw_span names on the materialised batch; _multi names it in
    indices of the whole set."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = W.Rng(71)
    queries = [b"", b"", b""] + [rand_seq(rng, 40 + 13 * i, DNA) for i in range(12)]
    queries[5] = plant_x(queries[5], 20)
    targets = [rand_seq(rng, 30 + 7 * j, DNA) for j in range(16)]
    targets[9] = plant_x(targets[9], 10)
    want = (3, 9)
    if long_query:
        queries[1] = plant_x(rand_seq(rng, 700, DNA), 600)
        want = (1, 0)
    q, t = W.seqset_from(queries), W.seqset_from(targets)
    with pytest.raises(S.SeqAlignError) as err:
        ctx.sw_span_cross(q, t, hyb)
    assert named_pair(err) == want == pairwise_pair(ctx, q, t, hyb)
    with S.Context(0) as peer:
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_span_cross(W.seqset_from([b""] * 4 + queries), t, hyb, peers=[peer])
    assert named_pair(err) == (want[0] + 4, want[1])
    ok = ctx.sw_span_cross(W.seqset_from(queries[6:8]), W.seqset_from(targets[:3]), S.make_scoring(DNA_SW))
    assert ok[0].shape == (2, 3)                                  # the context still works


def test_unknown_pair_across_tiles(ctx):
    """chunk_bytes = 1 MiB and 3 000 more targets: two target ranges.  X in query 8 fails (8, 0) in the first range, X in
    target 2 916 fails (3, 2 916) in the second: the lower pair, found in the later tile, is the one named -- as without
    tiles."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    rng = W.Rng(75)
    queries = [b"", b"", b""] + [rand_seq(rng, 40 + 13 * i, DNA) for i in range(12)]
    queries[8] = plant_x(queries[8], 3)
    filler = W.random_set(3000, 76, 150, 250, DNA)
    targets = [rand_seq(rng, 30 + 7 * j, DNA) for j in range(16)] + [filler.seq(j) for j in range(3000)]
    targets[2916] = plant_x(targets[2916], 100)
    q, t = W.seqset_from(queries), W.seqset_from(targets)
    with pytest.raises(S.SeqAlignError) as err_one:
        ctx.sw_span_cross(q, t, hyb)
    with ctx.options(chunk_bytes=1 << 20):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_span_cross(q, t, hyb)
        assert ctx.last_call()["score_cross"][0] >= 2
    assert named_pair(err) == named_pair(err_one) == (3, 2916)


# ---------------------------------------------------------------- 6. nothing to find --
def test_empty_sets_and_empty_matrices(ctx):
    sc = S.make_scoring(DNA_SW)
    none, some = W.seqset_from([]), W.seqset_from([b"ACGT", b"GG"])
    assert all(x.shape == (0, 2) for x in ctx.sw_span_cross(none, some, sc))
    assert all(x.shape == (2, 0) for x in ctx.sw_span_cross(some, none, sc))
    assert ctx.last_call() == {}
    with S.Context(0) as peer:
        assert ctx.sw_span_cross(some, none, sc, peers=[peer])[0].shape == (2, 0)
    # sets of empty sequences, and sequences that share no letter: five matrices of zeros, written over what was there
    for q, t in ((W.seqset_from([b"", b""]), W.seqset_from([b"", b"", b""])), (W.seqset_from([b"", b"ACGT"]), W.seqset_from([b""])),
                 (W.seqset_from([b"AAAA", b"CACA" * 40, b"A" * 600]), W.seqset_from([b"GGTG", b"T" * 90]))):
        got = ctx.sw_span_cross(q, t, sc)
        assert all(x.shape == (q.n_seqs, t.n_seqs) and not x.any() for x in got)
        assert_equal(got, explicit(ctx, q, t, sc))


# ---------------------------------------------------------------- 7. several contexts --
def test_multi_context_equals_single(ctx):
    rng = W.Rng(91)
    q = W.seqset_from([rand_seq(rng, n, DNA) for n in rng.below(520, 60).tolist()] + [rand_seq(rng, 1400, DNA)])
    t = W.random_set(200, 92, 0, 300, DNA)
    sc = S.make_scoring(DNA_SW)
    one = ctx.sw_span_cross(q, t, sc)
    with S.Context(0) as peer:
        two = ctx.sw_span_cross(q, t, sc, peers=[peer])
    assert_equal(two, one)


# ---------------------------------------------------------------- 8. magnitude --
def largest_admitted_scale(base, la, lb):
    """The largest s at which maglib.admitted (the documented rule, restated) accepts the base scoring times s."""
    lo, hi = 1, 2 ** 31
    assert G.admitted(G.scaled(G.BASES[base], lo), la, lb) and not G.admitted(G.scaled(G.BASES[base], hi), la, lb)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if G.admitted(G.scaled(G.BASES[base], mid), la, lb) else (lo, mid)
    return lo


@pytest.mark.parametrize("shape", ["c1", "c8", "strips"])
@pytest.mark.parametrize("base", ["steep", "extpos"])
def test_magnitude_at_the_edge_of_the_admitted_domain(ctx, base, shape):
    """maglib's pairs of one shape as sets (every seq_a against every seq_b).  The largest scale the documented rule admits:
    the matrices equal the oracle's first hits.  One more: SEQALIGN_E_DOMAIN before any launch."""
    pairs = [G.pair(shape, kind) for kind in G.kinds_of(shape)]
    q, t = W.seqset_from([a for a, _ in pairs]), W.seqset_from([b for _, b in pairs])
    la, lb = max(len(a) for a, _ in pairs), max(len(b) for _, b in pairs)
    s = largest_admitted_scale(base, la, lb)
    inside, outside = G.scaled(G.BASES[base], s), G.scaled(G.BASES[base], s + 1)
    got = ctx.sw_span_cross(q, t, S.make_scoring(inside))
    assert set(ctx.last_call()) == ({"score_strips"} if shape == "strips" else {"score_cross"})
    batch = W.cross_batch(q, t)
    assert [tuple(int(x.reshape(-1)[p]) for x in got) for p in range(batch.n_pairs)] == SP.want_spans(G.oracle_scoring(inside), batch)
    assert int(got[0].max()) > 2 ** 24
    with pytest.raises(S.SeqAlignError) as err:
        ctx.sw_span_cross(q, t, S.make_scoring(outside))
    assert err.value.code == S.E_DOMAIN and ctx.last_call() == {}
