"""GPU tier: SW hit spans (sa_span.hip) on gap-dense pairs, on tie-dense pairs and under the flags that change a row, in every
class of the span launcher: 1 .. 6 and 8 columns per lane of the one-wave rows kernel, and the strips kernel at two to five
strips of 512 columns.

tests/test_gpu_sw_span.py checks the widths with random DNA, the ties at len_a <= 140 (1 .. 3 columns per lane) and the flags
at len_a <= 140; tests/test_gpu_gap_dense.py runs the gap-dense families through sw_batch only.  Here the same hit is asked
of sw_span's own device code: GAP_A reached from GAP_B on every period of the pair (denselib.alternation, straddling, spaced),
ties that cross a seam of 512 columns (spanlib.tie_pairs), `forced`, the last-column exception of no_gaps_in_a and the blocked
cells of no_mismatches in the strips kernel (spanlib.flag_pairs).  tests/test_span_band_dense_argument_cpu.py argues on the
oracle alone that the pairs contain all that.  Every case compares all five outputs with spanlib.want_spans and asserts what
seqalign_ctx_last_call_info says ran.
"""
import itertools

import pytest

import denselib as D
import orclib as O
import seqalign_amd as S
import spanlib as SP
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

ROWS_CLASSES = 7      # columns per lane 1, 2, 3, 4, 5, 6, 8


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


_WANT = {}


def want_of(key, osc, pairs):
    """spanlib.want_spans, once per (scoring, pair) for the whole file."""
    new = [p for p in dict.fromkeys(pairs) if (key, p) not in _WANT]
    if new:
        for p, w in zip(new, SP.want_spans(osc, W.from_pairs(new))):
            _WANT[(key, p)] = w
    return [_WANT[(key, p)] for p in pairs]


def check(ctx, sc, osc, key, pairs, tag):
    """sw_span on the pairs against the oracle's first hits; returns what ran."""
    want = want_of(key, osc, pairs)
    got = SP.got_spans(ctx.sw_span(W.from_pairs(pairs), sc))
    ran = ctx.last_call()
    bad = [(p, len(pairs[p][0]), len(pairs[p][1]), got[p], want[p]) for p in range(len(pairs)) if got[p] != want[p]]
    assert not bad, (tag, len(bad), bad[:5], ran)
    return ran


def ran_one_class(ran, len_a, n):
    """One launch of the rows kernel (one class) or one of the strips kernel, nothing else."""
    return ran == ({"score_strips": (1, n)} if len_a > D.SPAN_STRIP_COLS else {"score_rows": (1, n)})


# ---------------------------------------------------------------- A1. gap-dense pairs in every launch class --
def dense_pairs(la, lb, name):
    return D.span_counted(la, lb, name) + D.span_seam(la, lb, name) + D.span_added(la, lb, name)


@pytest.mark.parametrize("shape", D.SPAN_ROWS_SHAPES + D.SPAN_STRIPS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", D.SW_SCORINGS)
def test_gap_dense_pairs_in_every_class(ctx, name, shape):
    """One shape per call: alternation k = 0 .. 7 (I->D on every period; at least 13 per hit), for rows of several strips the
    straddling pairs (the dense hit across column 512), and two spaced pairs."""
    la, lb = shape
    pairs = dense_pairs(la, lb, name)
    ran = check(ctx, S.make_scoring(D.SCORINGS[name]), D.oracle_scoring(name), name, pairs, (name, shape))
    assert ran_one_class(ran, la, len(pairs)), (name, shape, ran)


@pytest.mark.parametrize("name", D.SW_SCORINGS)
def test_gap_dense_pairs_every_class_in_one_call(ctx, name):
    """Every shape in one call: one launch per class of the rows kernel and one of the strips kernel."""
    rows = [p for la, lb in D.SPAN_ROWS_SHAPES for p in dense_pairs(la, lb, name)]
    strips = [p for la, lb in D.SPAN_STRIPS_SHAPES for p in dense_pairs(la, lb, name)]
    pairs = [p for two in itertools.zip_longest(rows, strips) for p in two if p is not None]      # interleaved
    ran = check(ctx, S.make_scoring(D.SCORINGS[name]), D.oracle_scoring(name), name, pairs, (name, "mixed"))
    assert set(ran) == {"score_rows", "score_strips"}, ran
    assert ran == {"score_rows": (ROWS_CLASSES, len(rows)), "score_strips": (1, len(strips))}, ran


# ---------------------------------------------------------------- A2. tie-dense pairs in every class --
@pytest.mark.parametrize("width", SP.TIE_ROWS_WIDTHS + SP.TIE_STRIPS_WIDTHS)
@pytest.mark.parametrize("name", list(SP.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_in_every_class(ctx, name, width):
    """40 pairs over a binary alphabet, half of them related by indels, len_a within 6 of the width.  First, on the CPU: the
    shares test_span_band_dense_argument_cpu.py asserts -- reversing the predecessor priority (M > B > A) changes the span of
    at least 10 % of the pairs ([2,-1,0,-1], [3,-1,-1,0]) or 50 % ([2,-3,-2,1], whose floor pays), and for rows of several
    strips at least 25 % of the hits cross a multiple of 512 -- so a kernel with the wrong tie order at 4 .. 8 columns per
    lane, or at a strip seam, cannot pass."""
    spec = {"init": SP.TIE_SCORINGS[name] + [0] * 6}
    sc = S.make_scoring(spec)
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    pairs = SP.tie_pairs(name, width)
    both = [SP.walk_both(osc, a, b) for a, b in pairs]
    sensitive, across = sum(w != r for w, r in both), sum(SP.crosses_seam(w) for w, r in both)
    print(f"{name} width {width}: tie_sensitive {sensitive} of {len(pairs)}, seam-crossing hits {across}")
    assert sensitive >= (len(pairs) // 2 if name == "ext_pos" else len(pairs) // 10), sensitive
    assert width <= 512 or across >= len(pairs) // 4, across
    ran = check(ctx, sc, osc, ("tie", name), pairs, (name, width))
    assert [w for w, r in both] == want_of(("tie", name), osc, pairs)      # the walk the shares were counted with is the oracle's
    assert ran_one_class(ran, width, len(pairs)), (name, width, ran)


@pytest.mark.parametrize("name,width", [(n, w) for n in SP.SEAM_SCORINGS for w in SP.SEAM_WIDTHS[n]])
def test_ties_at_a_strip_seam(ctx, name, width):
    """24 pairs whose hit leaves a seam column diagonally out of a cell where gap_a and gap_b tie and lead to different
    starts (spanlib.seam_pairs): A > B there rests on the one bit the left strip hands on.  On the CPU first: at least half
    of the spans (a quarter under [2,-3,-2,1]) change when gap_b wins that tie on the steps across a seam only."""
    sc = S.make_scoring({"init": SP.SEAM_SCORINGS[name] + [0] * 6})
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    pairs = SP.seam_pairs(name, width)
    walks = [SP.walk_seams(osc, a, b) for a, b in pairs]
    telling = sum(w[0] != w[1] for w in walks)
    print(f"{name} width {width}: {telling} of {len(pairs)} spans change with the tie order lost at a seam")
    assert telling >= (len(pairs) // 4 if name == "ext_pos" else len(pairs) // 2), telling
    ran = check(ctx, sc, osc, ("seam", name), pairs, (name, width))
    assert [w[0] for w in walks] == want_of(("seam", name), osc, pairs)
    assert ran == {"score_strips": (1, len(pairs))}, (name, width, ran)


# ---------------------------------------------------------------- A3. the flags that matter, on wide rows --
def flag_case(ctx, flags, key):
    sc = S.make_scoring(SP.flag_spec(*flags))
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    every = []
    for width in SP.FLAG_WIDTHS:
        pairs = SP.flag_pairs(width)
        ran = check(ctx, sc, osc, key, pairs, (flags, width))
        assert ran == {"score_strips": (1, 4)}, (flags, width, ran)
        every += pairs
    ran = check(ctx, sc, osc, key, every, (flags, "all widths"))      # two, three and four strips in one grid
    assert ran == {"score_strips": (1, len(every))}, (flags, ran)
    return want_of(key, osc, every)


@pytest.mark.parametrize("flags", list(itertools.product([0, 1], repeat=3)), ids=lambda f: "".join(map(str, f)))
def test_row_flags_in_the_strips_kernel(ctx, flags):
    """no_gaps_in_a, no_gaps_in_b, no_mismatches (mismatch -6 where both no-gaps flags are set) at len_a 513, 700, 1 025, 1 100
    and 1 537: per width a hit that reaches the last column (no_gaps_in_a's exception), one that ends on the last row
    (no_gaps_in_b's), one in the middle and an unrelated pair.  Each non-zero combination changes 12 .. 15 of the 20 spans."""
    want = flag_case(ctx, flags, ("flags", flags))
    if any(flags):
        plain = want_of(("flags", (0, 0, 0)), O.Scoring.from_buffer_copy(bytes(S.make_scoring(SP.flag_spec()))),
                        [p for width in SP.FLAG_WIDTHS for p in SP.flag_pairs(width)])
        assert sum(x != y for x, y in zip(want, plain)) >= 5


def test_free_start_and_end_gaps_in_the_strips_kernel(ctx):
    """no_start_gap_penalty and no_end_gap_penalty, the four combinations, on the same pairs: the spans are the flag-free ones
    (a free end gap lies in the last column or row, and no match cell follows it), the free last row and column are computed."""
    spans = [flag_case(ctx, (0, 0, 0, *ends), ("ends", ends)) for ends in itertools.product([0, 1], repeat=2)]
    assert spans[1] == spans[2] == spans[3] == spans[0]
