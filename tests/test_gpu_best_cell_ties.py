"""GPU tier: the hit order of the SW best cell -- score descending, column ascending, row ascending
(smith_waterman.c:71-86) -- on ties planted on purpose, through every picker that has tie code of its own:

    sw_score, sw_score_cross, sw_score_search    BestCells::row / ::reduce (sa_strips.hpp) in score_rows / score_cross,
                                                 merge_left_best across the strips of score_strips
    sw_align_long                                the same in the long forward pass
    sw_batch(max_hits = 1)                       the packed best-hit fills, two and four pairs per wave; sa_reduce behind
                                                 the three-matrix path

seq_a is background over K, L and seq_b over M, N, which match nothing.  Planted into both are single letters (so that tied
columns can be adjacent) or 24-letter ACGT words:

    cross        X ends at column i1 and row j2, Y at column i2 > i1 and row j1 < j2: the best cells are (i1, j2) and
                 (i2, j1); column first gives (i1, j2), a row-first or last-wins picker (i2, j1)
    same column  X once in seq_a, twice in seq_b: the lower row wins
    same row     X twice in seq_a, once in seq_b: the lower column wins

The reference is the oracle, and for every pair the oracle's match_scores alone must show the tie that was meant: the maximum
at exactly the planted cells.  Placements: one len_a on each rung of the columns-per-lane ladder, at its widest row -- 64 CPL
columns for the score kernels, 64 CPL - 1 for the fills, whose row includes the border column -- with the tied columns in two
slots of a lane, in the last slot of a lane and the first of the next (adjacent columns around a multiple of CPL cover both
for either mapping of columns to lanes), and in the first and last lane; tied rows in one 64-row chunk, on either side of rows
64 | 65, and at rows 1 and len_b.  Past 1 024 columns: inside a strip, on either side of the strip edges, in the first and
the last strip, and one pair each where the left and the right strip hold the strictly higher cell.
"""
import functools
import random

import numpy as np
import pytest

import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W
from test_gpu_score import want_from_matrices
from test_gpu_score_search import assert_hits, top_k

pytestmark = pytest.mark.gpu

SPEC = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}
LADDER = (1, 2, 3, 4, 5, 6, 8, 12, 16)
ROW_LENS = sorted([64 * c for c in LADDER] + [64 * c - 1 for c in LADDER])
STRIP_LENS = [1025, 1600]
LEN_B = (90, 150)
WORD = 24


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def column_pairs(la):
    """(i1, i2), i1 < i2, 1-based."""
    if la > 1024:        # strips of 512 columns
        return [(100, 300), (512, 513), (1024, 1025), (30, la), (500, 540), (la - 60, la - 30)]
    cpl = next(c for c in LADDER if 64 * c >= la)
    m = 20 * cpl
    pairs = [(m - 1, m), (m, m + 1), (m + 1, m + 2), (1, la)]
    if la >= 128:
        pairs.append((la // 4, 3 * la // 4))
    return pairs


def row_pairs(lb):
    return [(30, 60), (64, 65), (1, lb), (30, 100 if lb > 100 else lb)]


def build(rng, la, lb, kind, cols, rows):
    """(a, b, the cells (column, row) that must hold the maximum, the one that must win, the length of the planted words,
    the cell that must hold the next lower value or None)."""
    (i1, i2), (j1, j2) = cols, rows
    a = bytearray(rng.choice(b"KL") for _ in range(la))
    b = bytearray(rng.choice(b"MN") for _ in range(lb))
    n = WORD if min(i1, j1) >= WORD and i2 - i1 >= WORD and j2 - j1 >= WORD else 1
    X, Y = (b"A", b"C") if n == 1 else (bytes(rng.choice(b"ACGT") for _ in range(n)) for _ in range(2))

    def plant(seq, end, word):
        assert end - len(word) >= 0 and end <= len(seq)
        seq[end - len(word):end] = word

    if kind == "cross":
        plant(a, i1, X); plant(a, i2, Y); plant(b, j1, Y); plant(b, j2, X)
        cells, win = [(i1, j2), (i2, j1)], (i1, j2)
    elif kind.startswith("same_column"):
        i = i1 if kind.endswith("1") else i2
        plant(a, i, X); plant(b, j1, X); plant(b, j2, X)
        cells, win = [(i, j1), (i, j2)], (i, j1)
    elif kind == "same_row":
        j = j2
        plant(a, i1, X); plant(a, i2, X); plant(b, j, X)
        cells, win = [(i1, j), (i2, j)], (i1, j)
    else:                # no tie: one strip holds the strictly higher cell, the other a cell one letter short of it
        assert n == WORD
        hi, lo = ((i1, j2), (i2, j1)) if kind == "left_higher" else ((i2, j1), (i1, j2))
        plant(a, hi[0], X); plant(b, hi[1], X); plant(a, lo[0], Y[1:]); plant(b, lo[1], Y[1:])
        return bytes(a), bytes(b), [hi], hi, n, lo
    return bytes(a), bytes(b), cells, win, n, None


@functools.lru_cache(maxsize=None)
def tie_batch(la, lb):
    """The pairs of one shape with what the oracle says of them, after the reference-only conditions: built once per shape."""
    rng = random.Random(1000 * la + lb)
    sc = S.make_scoring(SPEC)
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    pairs, kinds, want_score, want_hit = [], [], [], []
    specs = [(kind, cols, rows) for cols in column_pairs(la) for rows in row_pairs(lb)
             for kind in ("cross", "same_column_1", "same_column_2", "same_row")]
    if la > 1024:
        specs += [(kind, cols, (30, 70)) for kind in ("left_higher", "right_higher") for cols in ((100, 900), (500, 540), (1000, la))]
    for kind, cols, rows in specs:
        a, b, cells, win, n, lower = build(rng, la, lb, kind, cols, rows)
        rc, M, A, B = O.oracle_fill(osc, a, b, 1)
        assert rc == 0
        Mr = M.reshape(lb + 1, la + 1)
        at = sorted((int(c), int(r)) for r, c in zip(*np.nonzero(Mr == Mr.max())))
        tag = (la, lb, kind, cols, rows)
        assert at == sorted(cells), (tag, at, cells)                     # the maximum is at exactly the planted cells
        assert int(Mr.max()) == 2 * n, tag
        if lower is not None:                                            # no tie: the other strip's best is one letter lower
            assert len(at) == 1 and Mr[lower[1], lower[0]] == 2 * n - 2 and (lower[0] - 1) // 512 != (win[0] - 1) // 512, tag
            assert (kind == "left_higher") == (win[0] < lower[0]), tag
        else:
            (c1, r1), (c2, r2) = cells
            assert len(at) == 2, tag
            assert {"cross": c1 < c2 and r1 > r2, "same_column": c1 == c2 and r1 != r2,
                    "same_row": r1 == r2 and c1 != c2}[kind.rstrip("_12")], tag   # they differ in the coordinate that was meant
        want = want_from_matrices(M, A, B, la, lb, 1)
        assert want == (int(Mr.max()), *win), (tag, want, win)
        rc, hits = O.oracle_sw(osc, a, b, 1, 1)
        assert rc == 0 and len(hits) == 1 and (hits[0]["pos_a"] + hits[0]["len_a"], hits[0]["pos_b"] + hits[0]["len_b"]) == win, tag
        pairs.append((a, b)); kinds.append(tag); want_score.append(want); want_hit.append(hits)
    return sc, pairs, kinds, want_score, want_hit


def mismatches(got, want, kinds):
    return [(kinds[p], got[p], want[p]) for p in range(len(want)) if got[p] != want[p]]


def test_the_planted_ties_cover_what_they_should():
    """Counts, on the reference alone (tie_batch asserts the conditions pair by pair)."""
    n = {"cross": 0, "same_column": 0, "same_row": 0, "higher": 0, "word": 0, "letter": 0}
    for la in ROW_LENS + STRIP_LENS:
        for lb in LEN_B:
            _, pairs, kinds, want_score, _ = tie_batch(la, lb)
            for (_, _, kind, _, _), w in zip(kinds, want_score):
                n["higher" if kind.endswith("higher") else kind.rstrip("_12")] += 1
                n["word" if w[0] >= 2 * (WORD - 1) else "letter"] += 1
    print("planted pairs:", n)
    assert n["cross"] >= 300 and n["same_column"] >= 600 and n["same_row"] >= 300 and n["higher"] == 24 and n["word"] >= 100, n


@pytest.mark.parametrize("la", ROW_LENS + STRIP_LENS)
def test_sw_score(ctx, la):
    for lb in LEN_B:
        sc, pairs, kinds, want, _ = tie_batch(la, lb)
        s, ea, eb = ctx.sw_score(W.from_pairs(pairs), sc)
        assert set(ctx.last_call()) == ({"score_strips"} if la > 1024 else {"score_rows"}), ctx.last_call()
        got = [(int(s[p]), int(ea[p]), int(eb[p])) for p in range(len(pairs))]
        bad = mismatches(got, want, kinds)
        assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("la", ROW_LENS + STRIP_LENS)
def test_sw_score_cross_and_search(ctx, la):
    """Every seq_a against every seq_b of the batch: the pairs themselves are the diagonal, checked against the oracle; the
    search's three best targets per query are the lexsort of the cross call's matrix, with its ends."""
    for lb in LEN_B:
        sc, pairs, kinds, want, _ = tie_batch(la, lb)
        assert len({a for a, _ in pairs}) == len(pairs) == len({b for _, b in pairs})
        q, t = W.seqset_from([a for a, _ in pairs]), W.seqset_from([b for _, b in pairs])
        s, ea, eb = ctx.sw_score_cross(q, t, sc)
        assert set(ctx.last_call()) == ({"score_strips"} if la > 1024 else {"score_cross"}), ctx.last_call()
        got = [(int(s[p, p]), int(ea[p, p]), int(eb[p, p])) for p in range(len(pairs))]
        bad = mismatches(got, want, kinds)
        assert not bad, (len(bad), bad[:6])
        found = ctx.sw_score_search(q, t, sc, 3)
        # (rows of more than 1 024 columns come home through the score batches: their top k is taken on the host)
        assert set(ctx.last_call()) == ({"score_strips"} if la > 1024 else {"score_cross", "score_select"}), ctx.last_call()
        assert_hits(found, top_k(s, ea, eb, 3, 1), (la, lb))
        assert all(int(found[1][p, 0]["score"]) >= want[p][0] for p in range(len(pairs)))


@pytest.mark.parametrize("rows", [0, 17])
@pytest.mark.parametrize("la", ROW_LENS + STRIP_LENS)
def test_sw_align_long(ctx, la, rows):
    for lb in LEN_B:
        sc, pairs, kinds, _, want = tie_batch(la, lb)
        with ctx.options(long_block_rows=rows):
            got = ctx.sw_align_long(W.from_pairs(pairs), sc, 1)
            ran = ctx.last_call()
        assert "long_forward" in ran and set(ran) <= {"long_forward", "long_block", "long_walk"}, ran
        bad = mismatches(got, want, kinds)
        assert not bad, (len(bad), bad[:4])


PACKED = {"fill_sw_best_x2", "fill_sw_best_x4"}


@pytest.mark.parametrize("la", ROW_LENS + STRIP_LENS)
def test_sw_batch_best_hit(ctx, la):
    """sw_batch(max_hits = 1): two pairs per wave, four pairs per wave (rows up to 191 columns; 4 k + 3 and 4 k + 1 pairs, so
    the last wave holds three and one), the three-matrix path, and whatever the defaults choose."""
    for lb in LEN_B:
        sc, pairs, kinds, _, want = tie_batch(la, lb)
        n = len(pairs)
        assert n % 4 == 0 or la > 1024

        def run(count, **opts):
            with ctx.options(**opts):
                got = ctx.sw_batch(W.from_pairs(pairs[:count]), sc, 1, max_hits=1)
                ran = ctx.last_call()
            bad = mismatches(got, want[:count], kinds)
            assert not bad, (opts, count, len(bad), bad[:4])
            return set(ran)

        for count in (n, n - 1):
            ran = run(count, pack16=2, quad=1)
            assert (("fill_sw_best_x2" in ran) == (la <= 1023)) and "fill_sw_best_x4" not in ran, (la, ran)
        if la <= 191:
            for count in (n - n % 4 - 1, n - n % 4 - 3):
                assert run(count, pack16=2, quad=2) & PACKED == {"fill_sw_best_x4"}
        ran = run(n, pack16=0)
        assert not ran & PACKED, ran
        run(n)
