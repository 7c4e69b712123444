"""GPU tier: banded SW hit spans -- seqalign_sw_span_banded (sa_band_span.hip, sa_batch_band.hip).

Every case is compared bit for bit with the oracle: the five fields of bandswlib.expected's hit (min_score = 1), zeros without
one; and score and pos + len must equal ctx.sw_score_banded on the same batch.  Shapes are test_gpu_band_sw.py's, the smallest
at which the frame can go wrong: 130-200 rows, so the frame moves across two 64-row code fetches; every width at which the
columns per lane step up, both sides of it; bands left of, right of and across the main diagonal, off the right side, off the
bottom, outside the pair; a gap that pays, whose hits start outside the band; tie-dense pairs; planted ties of the maximum
that the moving frame's best-cell bookkeeping has to order, spans included; every kind of scoring the sweep has a path for."""
import itertools
import random

import numpy as np
import pytest

import bandspanlib as BSP
import bandswlib as BS
import orclib as O
import seqalign_amd as S
import spanlib as SP
from seqalign_amd import workloads as W
from test_gpu_band_sw import PLAIN, SCORINGS, assert_maxima, planted, scoring

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512]
LADDER = [64, 128, 192, 256, 320, 384, 512]          # widths at which the columns per lane step up
WIDTH_SCORINGS = {"plain": (PLAIN, b"ACGT"), "ext0": ([3, -1, -1, 0], b"AC"), "ext_pos": ([2, -3, -2, 1], b"ACGT")}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def per_pair(x, n):
    return [x] * n if np.isscalar(x) else list(x)


def check(ctx, sc, osc, pairs, lo, hi, batch=None):
    """The span call on the batch against the oracle's banded hit, and against the banded score call; returns the wanted
    [(score cell, five fields)]."""
    n = len(pairs)
    lo, hi = per_pair(lo, n), per_pair(hi, n)
    want = [BSP.want(osc, a, b, lo[p], hi[p]) for p, (a, b) in enumerate(pairs)]
    batch = batch or W.from_pairs(pairs)
    res = ctx.sw_span_banded(batch, sc, lo, hi)
    got = SP.got_spans(res)
    bad = [(p, lo[p], hi[p], got[p], want[p][1]) for p in range(n) if got[p] != want[p][1]]
    assert not bad, (len(bad), bad[:3])
    score, end_a, end_b = ctx.sw_score_banded(batch, sc, lo, hi)
    ends = [(int(score[p]), int(end_a[p]), int(end_b[p])) for p in range(n)]
    assert ends == [(g[0], g[1] + g[3], g[2] + g[4]) for g in got] == [w[0] for w in want]
    return want


def n_hits(want):
    return sum(1 for cell, span in want if span[0] > 0)


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
    unbanded = SP.want_spans(osc, batch)
    full = ctx.sw_span(batch, sc)
    for lo, hi in ((-10 ** 6, 10 ** 6), (-2 ** 31, 2 ** 31 - 1)):
        want = check(ctx, sc, osc, pairs, lo, hi)
        assert [span for cell, span in want] == unbanded
        got = ctx.sw_span_banded(batch, sc, lo, hi)
        assert all(np.array_equal(g, f) for g, f in zip(got, full))


def test_empty_bands_and_empty_sequences(ctx):
    sc, osc = scoring(PLAIN)
    a, b = b"ACGTTGCAAGCTTGCA" * 3, b"GGACGTTGCAAGCTTGCATT" * 2
    la, lb = len(a), len(b)
    pairs = [(a, b), (a, b), (a, b), (a, b), (b"", b), (a, b""), (b"", b""), (a, b), (a, b)]
    lo = [la + 1, -lb - 9, la, -lb, -3, -3, 0, 2 ** 31 - 1, -2 ** 31]
    hi = [la + 70, -lb - 1, la, -lb, 3, 3, 0, 2 ** 31 - 1, -2 ** 31]
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert all(cell == (0, 0, 0) and span == BSP.ZEROS for cell, span in want)
    # ... next to pairs that do have a hit, and 1 x 1 pairs
    mixed = [pairs[0], (a, b), pairs[4], (a, b), pairs[6], (b"A", b"A"), (b"A", b"C"), (b"A", b"A")]
    want = check(ctx, sc, osc, mixed, [la + 1, -4, -3, -40, 0, 0, 0, 1], [la + 70, 4, 3, 40, 0, 0, 0, 1])
    assert [span[0] > 0 for cell, span in want] == [False, True, False, True, False, True, False, False]
    assert want[5][1] == (PLAIN[0], 0, 0, 1, 1)


# ---------------------------------------------------------------- 4. the start outside the band --
def test_a_gap_that_pays_starts_hits_outside_the_band(ctx):
    """Reads in windows under gap_extend = +1: the walk steps onto a cell outside the band, which reads 0, and stops there."""
    rng = random.Random(404)
    sc, osc = scoring([2, -3, -2, 1])
    pairs, lo, hi = [], [], []
    for _ in range(40):
        read, window, offset = BS.read_in_window(rng, 150, 200, 0.08)
        pairs.append((read, window))
        lo.append(-offset - 4)
        hi.append(-offset + 4)
    want = check(ctx, sc, osc, pairs, lo, hi)
    outside = sum(BSP.starts_outside(span, len(a), len(b), lo[p], hi[p]) for p, ((a, b), (cell, span)) in enumerate(zip(pairs, want)))
    print("starts outside the band:", outside, "of", n_hits(want))
    assert outside >= 10, outside


# ---------------------------------------------------------------- 5. ties --
@pytest.mark.parametrize("band", BSP.TIE_BANDS)
@pytest.mark.parametrize("width", BSP.TIE_WIDTHS)
@pytest.mark.parametrize("name", list(SP.TIE_SCORINGS))
def test_ties_follow_the_walkers_order_inside_a_band(ctx, name, width, band):
    """spanlib.tie_pairs' batches (bandspanlib.tie_batch); that each holds a pair whose wanted span changes under the reversed
    priority is asserted on the oracle in test_sw_span_banded_argument_cpu.py."""
    sc, osc = scoring(SP.TIE_SCORINGS[name])
    want = check(ctx, sc, osc, BSP.tie_batch(name, width), *band)
    assert n_hits(want) >= 30, n_hits(want)


# ---------------------------------------------------------------- 6. best-cell ties across the moving frame --
def planted_words(rng, la, lb, places):
    """seq_a = A's, seq_b = T's, which match nothing; per (p, q, word id, L) of `places` a random C/G word of L letters at
    seq_a[p:] and at seq_b[q:], the same word for the same id: a copy scores 2 L at its end cell (p + L, q + L), and its span
    is (p, q, L, L)."""
    words = {}
    a, b = bytearray(b"A" * la), bytearray(b"T" * lb)
    for p, q, w, L in places:
        while w not in words:
            cand = bytes(rng.choice(b"CG") for _ in range(L))
            if all(sum(x != y for x, y in zip(cand, o)) >= L // 3 for o in words.values()):
                words[w] = cand
        assert len(words[w]) == L
        a[p:p + L] = words[w]
        b[q:q + L] = words[w]
    return bytes(a), bytes(b)


TIES = {
    # name: (lo, hi, la, lb, places, the index of the copy that wins)
    # (a) the lower column has long left the frame when the later copy peaks (test_gpu_band_sw.py's construction)
    "retired, narrow band": (-4, 4, 128, 150, [(10, 10, 0, 20), (93, 89, 0, 20)], 0),
    "retired, frame of one lane row": (-60, 3, 160, 150, [(10, 10, 0, 20), (117, 115, 0, 20)], 0),
    "retired, three columns per lane": (-110, 20, 220, 175, [(10, 10, 0, 20), (160, 145, 1, 20)], 0),
    # ... and leaves through lane 0 on the very row the later one peaks
    "retires on that row": (-60, 3, 120, 131, [(10, 10, 0, 20), (41, 71, 1, 20)], 0),
    # (b) two live columns tie: the lower column wins, whichever row it is on
    "live, lower column on the lower row": (-60, 3, 170, 165, [(100, 110, 0, 12), (120, 150, 1, 12)], 0),
    "live, lower column on the higher row": (-60, 20, 170, 165, [(100, 150, 0, 12), (120, 110, 1, 12)], 0),
    "live, columns 13 apart": (-60, 20, 170, 165, [(100, 150, 0, 12), (113, 100, 1, 12)], 0),
    # (c) one column reaches the same score on two rows: the lower row wins; the column's position moves in between
    "one column, rows 14 apart": (3, 23, 160, 150, [(90, 70, 0, 12), (90, 84, 0, 12)], 0),
    "one column, rows 40 apart": (-23, 23, 160, 150, [(90, 70, 0, 12), (90, 110, 0, 12)], 0),
    # three copies: one retired, two live; and a retired copy one letter short of two live ones
    "three copies": (-60, 3, 200, 190, [(10, 10, 0, 20), (110, 120, 1, 20), (150, 165, 2, 20)], 0),
    "three copies, the retired one a letter short": (-60, 3, 190, 190, [(11, 11, 0, 19), (110, 160, 1, 20), (135, 136, 2, 20)], 1),
}


@pytest.mark.parametrize("name", list(TIES))
def test_best_cell_ties_across_the_moving_frame(ctx, name):
    lo, hi, la, lb, places, win = TIES[name]
    rng = random.Random(len(name) * 7)
    sc, osc = scoring(PLAIN)
    a, b = planted_words(rng, la, lb, places)
    L = max(pl[3] for pl in places)
    cells = sorted({(p + n, q + n) for p, q, w, n in places if n == L})
    assert 130 <= len(b) <= 200 and len(cells) >= 2
    assert_maxima(osc, a, b, lo, hi, cells)               # on the oracle alone: the banded maximum stands at exactly these
    d_lo = max(lo, -lb)
    if name.startswith("retired") or name.startswith("three copies"):
        p0, _, _, n0 = places[0]
        assert max(r for c, r in cells) + d_lo > p0 + n0  # the first copy's column has left the frame by the last peak
    if name == "retires on that row":
        assert cells[1][1] + d_lo == cells[0][0] + 1
    if name.startswith("live"):
        assert min(lb, la - d_lo) + d_lo <= min(c for c, r in cells)      # both columns are in the last row's frame
    p, q = places[win][:2]
    want = check(ctx, sc, osc, [(a, b)], lo, hi)
    assert want[0] == ((2 * L, p + L, q + L), (2 * L, p, q, L, L)), (want, places[win])


# ---------------------------------------------------------------- 7. scorings --
@pytest.mark.parametrize("name", list(SCORINGS))
def test_scorings(ctx, name):
    """test_gpu_band_sw.py's scorings (BLOSUM62 on protein pairs, a wildcard, mutations and case, flags, a gap that pays), per
    scoring eight pairs over four width classes, bands on both sides of the diagonal."""
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
    """no_gaps_in_a, no_gaps_in_b, no_mismatches at width 385 on spanlib.flag_pairs(460): seq_b a relative of seq_a's last 90
    letters (the hit reaches the last column), of its first 90 (unchanged at their end: the hit ends on the last row), of 90
    letters around its middle, and unrelated."""
    sc = S.make_scoring(SP.flag_spec(*flags))
    osc = O.Scoring.from_buffer_copy(bytes(sc))
    pairs = SP.flag_pairs(460)
    lo, hi = -10, 374
    assert all(BS.width_of(len(a), len(b), lo, hi) == 385 for a, b in pairs)
    want = check(ctx, sc, osc, pairs, lo, hi)
    spans = [span for cell, span in want]
    assert n_hits(want) >= 3
    if not any(flags):
        assert spans[0][1] + spans[0][3] == 460 and spans[1][2] + spans[1][4] == len(pairs[1][1]), spans


# ---------------------------------------------------------------- 8. one long band --
def test_one_long_band(ctx):
    """3 000 x 3 000 at width 512 with 8 % edits: dozens of code fetches, the frame moving on all but 255 rows."""
    rng = random.Random(88)
    sc, osc = scoring(PLAIN)
    a, b = planted(rng, 3000, 3000, 0, 0.08)
    want = check(ctx, sc, osc, [(a, b)], -256, 255)
    assert want[0][1][0] > 2000 and want[0][1][3] > 2000, want


# ---------------------------------------------------------------- 9. mixed classes and chunks --
def class_of(width):
    return next(k for k, edge in enumerate(LADDER) if width <= edge)


def test_mixed_classes_in_one_call_and_in_three_chunks(ctx):
    """60 pairs from all seven width classes.  Three of them have a seq_a of 700 000 letters (and 3 rows), so that at
    chunk_bytes = 1 MiB -- a pair takes len_a + len_b + 88 bytes -- the batch is cut into three chunks."""
    rng = random.Random(9)
    sc, osc = scoring(PLAIN)
    widths = [1, 64, 65, 128, 130, 192, 200, 256, 300, 320, 350, 384, 400, 512, 2]
    pairs, lo, hi = [], [], []
    for k in range(60):
        w = widths[k % len(widths)]
        first = rng.randrange(-40, 10)
        if k in (10, 30, 50):
            w, first = 64, -2
            pairs.append(planted(rng, 700000, 3, 1, 0.0))
        else:
            pairs.append(planted(rng, first + w + 60, rng.randrange(130, 180), first + w // 2))
        lo.append(first)
        hi.append(first + w - 1)
        assert BS.width_of(len(pairs[-1][0]), len(pairs[-1][1]), lo[-1], hi[-1]) == w
    classes = [class_of(hi[k] - lo[k] + 1) for k in range(60)]
    assert set(classes) == set(range(7))
    batch = W.from_pairs(pairs)
    want = check(ctx, sc, osc, pairs, lo, hi, batch)
    assert n_hits(want) >= 50 and all(want[k][1][0] > 0 for k in (10, 30, 50))
    one = ctx.sw_span_banded(batch, sc, lo, hi)
    assert ctx.last_call() == {"band_score": (7, 60)}
    # the greedy cut of the contract: a chunk closes before the pair that would take it over the budget
    chunks, used = [[]], 0
    for k, (a, b) in enumerate(pairs):
        need = len(a) + len(b) + 88
        if chunks[-1] and used + need > (1 << 20):
            chunks.append([])
            used = 0
        chunks[-1].append(k)
        used += need
    assert len(chunks) == 3
    with ctx.options(chunk_bytes=1 << 20):
        got = ctx.sw_span_banded(batch, sc, lo, hi)
        info = ctx.last_call()
    assert info == {"band_score": (sum(len({classes[k] for k in c}) for c in chunks), 60)}, info
    assert all(np.array_equal(g, o) for g, o in zip(got, one))
    assert SP.got_spans(got) == [span for cell, span in want]


# ---------------------------------------------------------------- 10. unknown pair --
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
        ctx.sw_span_banded(inside, sc, -8, 8)
    assert got.value.code == S.E_UNKNOWN_PAIR and "pair 2:" in str(got.value), str(got.value)
    assert BS.fill_unknown(osc, with_x, near, (-8, 8))[3] == [(101, 104)]
    assert BS.fill_unknown(osc, with_x, far, (-8, 8))[3] == []
    want = check(ctx, sc, osc, [good, (with_x, far), good], -8, 8)
    assert n_hits(want) == 3


# ---------------------------------------------------------------- 11. timing hook --
def test_time_hook_times_one_chunk_and_refuses_two(ctx):
    sc, _ = scoring(PLAIN)
    batch = W.from_pairs([(b"ACGT" * 50, b"ACGTTACGTACGAT" * 14)] * 4000)   # 200 + 196 + 88 bytes per pair: 1.9 MB
    with ctx.options(chunk_bytes=1 << 20):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_span_band_time_ms(batch, sc, -10, 10, repeats=3)
    assert err.value.code == S.E_ARG and "seqalign_sw_span_band_time_ms: the batch does not fit one chunk" in str(err.value), str(err.value)
    ms = ctx.sw_span_band_time_ms(batch, sc, -10, 10, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms
