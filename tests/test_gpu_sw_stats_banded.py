"""GPU tier: banded SW statistics -- seqalign_sw_stats_banded (sa_band_stats.hip, sa_band_frame.hpp, sa_batch_band.hip).

Every case is compared bit for bit with the oracle: the seven values of bandswlib.expected's hit (min_score = 1) and the counted
columns of its strings (bandstatlib.want), zeros without one; the first five must equal ctx.sw_span_banded on the same batch,
and score and pos + len must equal ctx.sw_score_banded.  Shapes are test_gpu_sw_span_banded.py's, the smallest at which the
frame can go wrong: 130-200 rows, so the frame moves across two 64-row code fetches; every width at which the columns per lane
step up, both sides of it; bands on both sides of and across the main diagonal, off the right side, off the bottom, outside the
pair; a gap that pays, whose hits start outside the band with nothing counted there; tie-dense pairs whose COUNTS depend on the
walker's order; planted ties of the maximum across the moving frame; scorings under which counting is not scoring; and both
sequences at 65 535 letters, where the packed coordinates are largest and the frame overhangs len_a."""
import itertools
import random

import numpy as np
import pytest

import bandspanlib as BSP
import bandstatlib as BST
import bandswlib as BS
import orclib as O
import seqalign_amd as S
import spanlib as SP
import swstatlib as SS
from seqalign_amd import workloads as W
from test_gpu_band_sw import PLAIN, SCORINGS, assert_maxima, planted, scoring
from test_gpu_sw_span_banded import LADDER, TIES, WIDTH_SCORINGS, WIDTHS, class_of, planted_words

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def per_pair(x, n):
    return [x] * n if np.isscalar(x) else list(x)


def check(ctx, sc, osc, pairs, lo, hi, batch=None):
    """The statistics call on the batch against the oracle's banded hit and its counted strings, against the banded span call
    and against the banded score call; returns the wanted [(score cell, seven values)]."""
    n = len(pairs)
    lo, hi = per_pair(lo, n), per_pair(hi, n)
    want = [BST.want(osc, a, b, lo[p], hi[p]) for p, (a, b) in enumerate(pairs)]
    batch = batch or W.from_pairs(pairs)
    res = ctx.sw_stats_banded(batch, sc, lo, hi)
    assert [r.dtype for r in res] == [np.int32] + [np.uint32] * 6 and all(r.shape == (n,) for r in res)
    got = BST.got_stats(res)
    bad = [(p, lo[p], hi[p], got[p], want[p][1]) for p in range(n) if got[p] != want[p][1]]
    assert not bad, (len(bad), bad[:3])
    span = ctx.sw_span_banded(batch, sc, lo, hi)
    assert all(np.array_equal(r, s) for r, s in zip(res[:5], span))
    score, end_a, end_b = ctx.sw_score_banded(batch, sc, lo, hi)
    ends = [(int(score[p]), int(end_a[p]), int(end_b[p])) for p in range(n)]
    assert ends == [(g[0], g[1] + g[3], g[2] + g[4]) for g in got] == [w[0] for w in want]
    return want


def n_hits(want):
    return sum(1 for cell, seven in want if seven[0] > 0)


# ---------------------------------------------------------------- 1. widths --
@pytest.mark.parametrize("name", list(WIDTH_SCORINGS))
@pytest.mark.parametrize("width", WIDTHS)
def test_every_width_class_and_its_edges(ctx, width, name):
    """Three pairs per width: the hit along the band's left edge, along its right edge, and in the middle; the band right of
    the main diagonal, left of it and across it."""
    init, alpha = WIDTH_SCORINGS[name]
    rng = random.Random(1000 + width)
    sc, osc = scoring(init)
    pairs, lo, hi = [], [], []
    for k, first in enumerate((7, -width - 5, -(width // 2))):
        lb = rng.randrange(130, 201)
        last = first + width - 1
        la = max(last, 0) + rng.randrange(40, 90)
        diag = (first, last, (first + last) // 2)[k]
        pairs.append(planted(rng, la, lb, diag, alphabet=alpha))
        lo.append(first)
        hi.append(last)
    assert BS.width_of(len(pairs[0][0]), len(pairs[0][1]), lo[0], hi[0]) == width     # pair 0's band is not clipped
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 2, want


# ---------------------------------------------------------------- 2. band positions --
@pytest.mark.parametrize("width", [5, 70, 300])
def test_band_positions(ctx, width):
    rng = random.Random(2000 + width)
    sc, osc = scoring(PLAIN)
    h = width // 2
    cases = {
        "across the main diagonal": (planted(rng, 170 + width, 160, 0), -h, width - 1 - h),
        "right of it": (planted(rng, 260 + width, 150, 40 + h), 40, 40 + width - 1),
        "left of it": (planted(rng, 140, 199, -30 - h), -30 - width + 1, -30),
        "left of it, from a late row": (planted(rng, 140, 199, -100), -100 - h, -100 - h + width - 1),
        "off the right side before the last row": (planted(rng, 90 + h, 190, 10 + h), 10, 10 + width - 1),
        "off the bottom": (planted(rng, 500 + width, 131, 60), 60 - h, 60 - h + width - 1),
        "clipped on the left": (planted(rng, 150, 140, -130), -140 - width, -125),
        "clipped on the right": (planted(rng, 150, 140, 120), 110, 150 + width),
    }
    pairs = [c[0] for c in cases.values()]
    want = check(ctx, sc, osc, pairs, [c[1] for c in cases.values()], [c[2] for c in cases.values()])
    assert n_hits(want) >= 6, want


# ---------------------------------------------------------------- 3. degenerate inputs --
def test_bounds_far_outside_a_small_pair_are_the_unbanded_call(ctx):
    rng = random.Random(77)
    sc, osc = scoring(PLAIN)
    pairs = [planted(rng, rng.randrange(1, 60), rng.randrange(1, 60), rng.randrange(-5, 6), 0.15) for _ in range(24)]
    batch = W.from_pairs(pairs)
    unbanded = SS.want_sw_stats(osc, pairs)
    full = ctx.sw_stats(batch, sc)
    for lo, hi in ((-10 ** 6, 10 ** 6), (-2 ** 31, 2 ** 31 - 1)):
        want = check(ctx, sc, osc, pairs, lo, hi)
        assert [seven for cell, seven in want] == unbanded
        got = ctx.sw_stats_banded(batch, sc, lo, hi)
        assert len(got) == len(full) == 7 and all(np.array_equal(g, f) for g, f in zip(got, full))


def test_empty_bands_and_empty_sequences(ctx):
    sc, osc = scoring(PLAIN)
    a, b = b"ACGTTGCAAGCTTGCA" * 3, b"GGACGTTGCAAGCTTGCATT" * 2
    la, lb = len(a), len(b)
    pairs = [(a, b), (a, b), (a, b), (a, b), (b"", b), (a, b""), (b"", b""), (a, b), (a, b)]
    lo = [la + 1, -lb - 9, la, -lb, -3, -3, 0, 2 ** 31 - 1, -2 ** 31]
    hi = [la + 70, -lb - 1, la, -lb, 3, 3, 0, 2 ** 31 - 1, -2 ** 31]
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert all(cell == (0, 0, 0) and seven == BST.ZEROS for cell, seven in want)
    # ... next to pairs that do have a hit, and 1 x 1 pairs
    mixed = [pairs[0], (a, b), pairs[4], (a, b), pairs[6], (b"A", b"A"), (b"A", b"C"), (b"A", b"A")]
    want = check(ctx, sc, osc, mixed, [la + 1, -4, -3, -40, 0, 0, 0, 1], [la + 70, 4, 3, 40, 0, 0, 0, 1])
    assert [seven[0] > 0 for cell, seven in want] == [False, True, False, True, False, True, False, False]
    assert want[5][1] == (PLAIN[0], 0, 0, 1, 1, 1, 0)
    full = ctx.sw_stats(W.from_pairs(mixed), sc)             # far bounds: array for array the unbanded call, zeros included
    got = ctx.sw_stats_banded(W.from_pairs(mixed), sc, -10 ** 6, 10 ** 6)
    assert all(np.array_equal(g, f) for g, f in zip(got, full))


# ---------------------------------------------------------------- 4. the start outside the band --
def test_a_gap_that_pays_starts_hits_outside_the_band(ctx):
    """Reads in windows under gap_extend = +1: the walk steps onto a cell outside the band, which reads 0, and stops there
    with nothing counted: the counts are those of the strings (check), which end at that cell."""
    rng = random.Random(404)
    sc, osc = scoring([2, -3, -2, 1])
    pairs, lo, hi = [], [], []
    for _ in range(40):
        read, window, offset = BS.read_in_window(rng, 150, 200, 0.08)
        pairs.append((read, window))
        lo.append(-offset - 4)
        hi.append(-offset + 4)
    want = check(ctx, sc, osc, pairs, lo, hi)
    outside = [p for p, ((a, b), (cell, seven)) in enumerate(zip(pairs, want))
               if BSP.starts_outside(seven[:5], len(a), len(b), lo[p], hi[p])]
    print("starts outside the band:", len(outside), "of", n_hits(want))
    assert len(outside) >= 10, len(outside)
    assert all(want[p][1][5] + want[p][1][6] > 0 for p in outside)


# ---------------------------------------------------------------- 5. ties --
@pytest.mark.parametrize("band", BST.TIE_BANDS)
@pytest.mark.parametrize("width", BST.TIE_WIDTHS)
@pytest.mark.parametrize("name", list(SP.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_inside_a_band(ctx, name, width, band):
    """bandstatlib.tie_batch; that each holds a pair whose wanted COUNTS change under the reversed priority is asserted on the
    oracle in test_sw_stats_banded_argument_cpu.py."""
    sc, osc = scoring(SP.TIE_SCORINGS[name])
    want = check(ctx, sc, osc, BST.tie_batch(name, width), *band)
    assert n_hits(want) >= 30, n_hits(want)


# ---------------------------------------------------------------- 6. best-cell ties across the moving frame --
@pytest.mark.parametrize("name", list(TIES))
def test_best_cell_ties_across_the_moving_frame(ctx, name):
    """test_gpu_sw_span_banded.TIES: the winning copy's counts are (L, 0), its own and not another copy's."""
    lo, hi, la, lb, places, win = TIES[name]
    rng = random.Random(len(name) * 7)
    sc, osc = scoring(PLAIN)
    a, b = planted_words(rng, la, lb, places)
    L = max(pl[3] for pl in places)
    cells = sorted({(p + n, q + n) for p, q, w, n in places if n == L})
    assert 130 <= len(b) <= 200 and len(cells) >= 2
    assert_maxima(osc, a, b, lo, hi, cells)               # on the oracle alone: the banded maximum stands at exactly these
    p, q = places[win][:2]
    want = check(ctx, sc, osc, [(a, b)], lo, hi)
    assert want[0] == ((2 * L, p + L, q + L), (2 * L, p, q, L, L, L, 0)), (want, places[win])


# ---------------------------------------------------------------- 7. counts are not scores --
COUNT_SCORINGS = {
    # case-insensitive on mixed-case letters, and a/c score as well as a match: counted as a mismatch all the same
    "case_insensitive": (dict(init=[3, -2, -5, -2, 0, 0, 0, 0, 0, 0], mutations=[["a", "c", 3], ["c", "a", 3]]), b"ACGTacgt"),
    # a wildcard that pays: N against A counts as a mismatch, N against N as a match
    "wildcard": (dict(init=[2, -3, -4, -1, 0, 0, 0, 0, 0, 0], wildcards=[["N", 1]]), b"ACGTN"),
    # no_mismatches lets a wildcard column through: it is counted by its letters
    "no_mismatches": (dict(init=[2, -3, -4, -1, 0, 0, 0, 0, 1, 0], wildcards=[["N", 1]]), b"ACGTN"),
}


def split_by_scores(osc, hit):
    """(columns of two letters whose substitution score is above 0, the other columns of two letters): the split the scores
    would suggest."""
    look = SP._Lookup(osc)
    cols = [(x, y) for x, y in zip(hit["a"].encode(), hit["b"].encode()) if x != 45 and y != 45]
    pos = sum(look(x, y) > 0 for x, y in cols)
    return pos, len(cols) - pos


@pytest.mark.parametrize("name", list(COUNT_SCORINGS))
def test_counts_are_not_scores(ctx, name):
    """Eight pairs over four width classes; in at least one the counted split differs from the scores' (on the oracle)."""
    spec, alpha = COUNT_SCORINGS[name]
    sc = S.make_scoring(spec)
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    rng = random.Random(len(name) * 17)
    pairs, lo, hi = [], [], []
    for k, width in enumerate((3, 30, 64, 129, 200, 40, 9, 333)):
        first = (5, -20, -70, -140, 12, -33, -9, -300)[k]
        lb = rng.randrange(130, 201)
        pairs.append(planted(rng, max(first + width, 0) + rng.randrange(50, 120), lb, first + width // 2, 0.12, alpha))
        lo.append(first)
        hi.append(first + width - 1)
    assert len({class_of(h - l + 1) for l, h in zip(lo, hi)}) >= 4
    differs = 0
    for p, (a, b) in enumerate(pairs):
        hit = BS.expected(osc, a, b, lo[p], hi[p], 1)[1]
        differs += hit is not None and split_by_scores(osc, hit) != SS.hit_fields(osc, [hit])[5:]
    assert differs >= 1, differs
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 6, want
    if name == "wildcard":                                     # the two statements of the contract, on the GPU itself
        one = ctx.sw_stats_banded(W.from_pairs([(b"N", b"A"), (b"N", b"N")]), sc, 0, 0)
        assert BST.got_stats(one) == [(1, 0, 0, 1, 1, 0, 1), (1, 0, 0, 1, 1, 1, 0)]


# ---------------------------------------------------------------- 8. scorings and flags --
@pytest.mark.parametrize("name", list(SCORINGS))
def test_scorings(ctx, name):
    """test_gpu_band_sw.py's scorings, per scoring eight pairs over four width classes, bands on both sides of the diagonal."""
    sc, osc, alpha = SCORINGS[name]()
    rng = random.Random(len(name) * 131)
    pairs, lo, hi = [], [], []
    for k, width in enumerate((3, 30, 64, 129, 200, 40, 9, 333)):
        first = (5, -20, -70, -140, 12, -33, -9, -300)[k]
        lb = rng.randrange(130, 201)
        pairs.append(planted(rng, max(first + width, 0) + rng.randrange(50, 120), lb, first + width // 2, 0.12, alpha))
        lo.append(first)
        hi.append(first + width - 1)
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 6, want


@pytest.mark.parametrize("idx", range(32))
def test_all_flag_combinations_at_width_70(ctx, idx):
    flags = list(itertools.product([0, 1], repeat=5))[idx]
    spec = BSP.flag_scoring(idx, flags)
    sc = S.make_scoring(spec)
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
    rng = random.Random(7000 + idx)
    pairs, lo, hi = [], [], []
    for k in range(8):
        first = (3, -69, -35, -120, 0, -10, 40, -200)[k]
        lb = rng.randrange(130, 201)
        la = (max(first + 70, 0) + rng.randrange(50, 120)) if k != 4 else 100       # pair 4: the band runs off the right side
        pairs.append(planted(rng, la, lb, first + (0, 69, 35, 20, 50, 30, 10, 60)[k], 0.12, alpha))
        lo.append(first)
        hi.append(first + 69)
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 5, want


@pytest.mark.parametrize("flags", list(itertools.product([0, 1], repeat=3)))
def test_flags_that_change_the_row_at_eight_columns_per_lane(ctx, flags):
    """no_gaps_in_a, no_gaps_in_b, no_mismatches at width 385 on spanlib.flag_pairs(460)."""
    sc = S.make_scoring(SP.flag_spec(*flags))
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    pairs = SP.flag_pairs(460)
    lo, hi = -10, 374
    assert all(BS.width_of(len(a), len(b), lo, hi) == 385 for a, b in pairs)
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert n_hits(want) >= 3


# ---------------------------------------------------------------- 9. one long band --
def test_one_long_band(ctx):
    """3 000 x 3 000 at width 512 with 8 % edits: dozens of code fetches, the frame moving on all but 255 rows."""
    rng = random.Random(88)
    sc, osc = scoring(PLAIN)
    a, b = planted(rng, 3000, 3000, 0, 0.08)
    want = check(ctx, sc, osc, [(a, b)], -256, 255)
    assert want[0][1][5] > 2000 and want[0][1][6] > 0, want


# ---------------------------------------------------------------- 10. the length limit --
TOP = SS.MAX_LEN


def limit_pair(case):
    """((seq_a, seq_b), lo, hi): one pair with a sequence of 65 535 letters and a short one of 180, and a hit of 120 letters
    (three of them substituted) between columns / rows 65 300 and 65 420 of the long one, on diagonal +-65 260.
    "a": len_a = 65 535, 180 rows, the band 65 250 .. 65 449: four columns per lane, so the frame of row j ends at column
         j + 65 505 and overhangs len_a from row 31 on, and the band itself runs off the right side from row 87 on -- while the
         hit is being swept (rows 41 .. 160).  Frame positions there compute columns above 65 535.
    "b": len_b = 65 535, 180 columns, the band -65 360 .. -65 161 at the bottom: rows 65 162 .. 65 535 are swept."""
    rng = random.Random(65 + len(case))
    core = bytes(rng.choice(b"GT") for _ in range(120))
    core2 = bytearray(core)
    for k in (30, 60, 90):
        core2[k] = ord("G") + ord("T") - core2[k]                    # G <-> T: a mismatch inside the hit
    long_ = bytearray(rng.choice(b"AC") for _ in range(TOP))
    short = bytearray(rng.choice(b"KM") for _ in range(180))
    long_[65300:65420] = core
    short[40:160] = core2
    if case == "a":
        return (bytes(long_), bytes(short)), 65250, 65449
    return (bytes(short), bytes(long_)), -65360, -65161


@pytest.mark.parametrize("case", ["a", "b"])
def test_packed_coordinates_at_the_length_limit(ctx, case):
    sc, osc = scoring(PLAIN)
    (a, b), lo, hi = limit_pair(case)
    assert max(len(a), len(b)) == TOP and min(len(a), len(b)) <= 200 and BS.width_of(len(a), len(b), lo, hi) == 200
    if case == "a":
        assert 31 + lo + 4 * 64 - 1 > TOP and 87 + hi > TOP          # the frame, then the band, pass len_a on early rows
    want = check(ctx, sc, osc, [(a, b)], lo, hi)
    score, pos_a, pos_b, len_a, len_b, matches, mismatches = want[0][1]
    pos, end = (pos_a, pos_a + len_a) if case == "a" else (pos_b, pos_b + len_b)
    assert pos > 65000 and end > 65000 and (score, matches, mismatches) == (2 * 117 - 3 * 3, 117, 3), want


# ---------------------------------------------------------------- 11. mixed classes and chunks --
def test_mixed_classes_in_one_call_and_in_three_chunks(ctx):
    """60 pairs from all seven width classes.  36 of them have a seq_a of 65 000 letters (and 3 rows) -- the length limit rules
    out the span test's three pairs of 700 000 -- so that at chunk_bytes = 1 MiB, where a pair takes len_a + len_b + 96 bytes,
    the batch of 2.4 MB is cut into three chunks."""
    rng = random.Random(9)
    sc, osc = scoring(PLAIN)
    widths = [1, 64, 65, 128, 130, 192, 200, 256, 300, 320, 350, 384, 400, 512, 2]
    pairs, lo, hi = [], [], []
    for k in range(60):
        w = widths[k % len(widths)]
        if k % 5 in (1, 2, 3):
            first = -2
            pairs.append(planted(rng, 65000, 3, 1, 0.0))
        else:
            first = rng.randrange(-40, 10)
            pairs.append(planted(rng, first + w + 60, rng.randrange(130, 180), first + w // 2))
        lo.append(first)
        hi.append(first + w - 1)
        assert BS.width_of(len(pairs[-1][0]), len(pairs[-1][1]), lo[-1], hi[-1]) == w
    classes = [class_of(hi[k] - lo[k] + 1) for k in range(60)]
    assert set(classes) == set(range(len(LADDER)))
    batch = W.from_pairs(pairs)
    want = check(ctx, sc, osc, pairs, lo, hi, batch)
    assert n_hits(want) >= 50, n_hits(want)
    one = ctx.sw_stats_banded(batch, sc, lo, hi)
    assert ctx.last_call() == {"band_score": (7, 60)}
    # the greedy cut of the contract: a chunk closes before the pair that would take it over the budget
    chunks, used = [[]], 0
    for k, (a, b) in enumerate(pairs):
        need = len(a) + len(b) + 96
        if chunks[-1] and used + need > (1 << 20):
            chunks.append([])
            used = 0
        chunks[-1].append(k)
        used += need
    assert len(chunks) == 3
    with ctx.options(chunk_bytes=1 << 20):
        got = ctx.sw_stats_banded(batch, sc, lo, hi)
        info = ctx.last_call()
    assert info == {"band_score": (sum(len({classes[k] for k in c}) for c in chunks), 60)}, info
    assert all(np.array_equal(g, o) for g, o in zip(got, one))
    assert BST.got_stats(got) == [seven for cell, seven in want]


# ---------------------------------------------------------------- 12. unknown pair --
def test_unknown_pair_inside_and_outside_the_band(ctx):
    """X (in seq_a) against Y (in seq_b) has no score; every other pair of letters has one."""
    sc = S.make_scoring({"preset": "DNA_hybridization",
                         "mutations": [["x", c, -1] for c in "acgt"] + [[c, "y", -1] for c in "acgt"]})
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    rng = random.Random(3)
    a, b = planted(rng, 180, 170, 0)
    with_x = a[:100] + b"X" + a[101:]
    near, far = b[:103] + b"Y" + b[104:], b[:20] + b"Y" + b[21:]      # X meets Y on diagonal 100 - 103, or 100 - 20
    good = (a, b)
    inside = W.from_pairs([good, good, (with_x, near), (with_x, far), good, (with_x, near)])
    with pytest.raises(S.SeqAlignError) as got:
        ctx.sw_stats_banded(inside, sc, -8, 8)
    assert got.value.code == S.E_UNKNOWN_PAIR and "pair 2:" in str(got.value), str(got.value)
    assert BS.fill_unknown(osc, with_x, near, (-8, 8))[3] == [(101, 104)]
    assert BS.fill_unknown(osc, with_x, far, (-8, 8))[3] == []
    want = check(ctx, sc, osc, [good, (with_x, far), good], -8, 8)
    assert n_hits(want) == 3


# ---------------------------------------------------------------- 13. the GPU's own align call --
def test_agrees_with_the_align_call_on_the_gpu(ctx):
    rng = random.Random(1313)
    sc, osc = scoring(PLAIN)
    pairs, lo, hi = [], [], []
    for _ in range(40):
        read, window, offset = BS.read_in_window(rng, 150, 200, 0.08)
        pairs.append((read, window))
        lo.append(-offset - 12)
        hi.append(-offset + 12)
    batch = W.from_pairs(pairs)
    hits = ctx.sw_align_banded(batch, sc, lo, hi, min_score=1)
    got = BST.got_stats(ctx.sw_stats_banded(batch, sc, lo, hi))
    assert got == [SS.hit_fields(osc, h) for h in hits]
    assert sum(g[0] > 0 for g in got) >= 35 and sum(g[6] > 0 for g in got) >= 20


# ---------------------------------------------------------------- 14. timing hook --
def test_time_hook_times_one_chunk_and_refuses_two(ctx):
    sc, _ = scoring(PLAIN)
    batch = W.from_pairs([(b"ACGT" * 50, b"ACGTTACGTACGAT" * 14)] * 4000)   # 200 + 196 + 96 bytes per pair: 1.9 MB
    with ctx.options(chunk_bytes=1 << 20):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_stats_band_time_ms(batch, sc, -10, 10, repeats=3)
    assert err.value.code == S.E_ARG and "seqalign_sw_stats_band_time_ms: the batch does not fit one chunk" in str(err.value), str(err.value)
    ms = ctx.sw_stats_band_time_ms(batch, sc, -10, 10, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms
