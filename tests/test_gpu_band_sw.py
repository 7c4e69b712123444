"""GPU tier: banded SW -- seqalign_sw_score_banded / seqalign_sw_align_banded (sa_band.hip, sa_batch_band.hip).

Every case is compared, score call and align call, with the definition's Python restatement walked by the oracle
(bandswlib.expected), bit for bit.  Shapes are the smallest at which the kernels can still go wrong: 130-200 rows, so the
frame moves across two 64-row code fetches; every width at which the columns per lane step up, both sides of it; bands left,
right and across the main diagonal, off the right side, off the bottom, outside the pair; planted ties of the maximum that the
moving frame's best-cell bookkeeping has to order; every kind of scoring the sweep has a path for."""
import ctypes as C
import json
import random
from pathlib import Path

import numpy as np
import pytest

import bandlib as BL
import bandswlib as BS
import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

LADDER = [64, 128, 192, 256, 320, 384, 512, 768, 1024]   # widths at which the columns per lane step up
WIDTHS = sorted({1, 2, 63} | set(LADDER) | {w + 1 for w in LADDER if w < 1024})
PLAIN = [2, -3, -4, -1]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def scoring(init, **more):
    sc = S.make_scoring({"init": [*init, *([0] * (10 - len(init)))], **more})
    return sc, O.Scoring.from_buffer_copy(bytes(sc))


def check(ctx, sc, osc, pairs, lo, hi, min_score=1):
    """Both calls on the batch against bandswlib.expected, pair by pair; returns the expected (score cell, hit) list."""
    n = len(pairs)
    lo = [lo] * n if np.isscalar(lo) else list(lo)
    hi = [hi] * n if np.isscalar(hi) else list(hi)
    want = [BS.expected(osc, a, b, lo[p], hi[p], min_score) for p, (a, b) in enumerate(pairs)]
    batch = W.from_pairs(pairs)
    score, end_a, end_b = ctx.sw_score_banded(batch, sc, lo, hi)
    got_cells = [(int(score[p]), int(end_a[p]), int(end_b[p])) for p in range(n)]
    bad = [(p, lo[p], hi[p], got_cells[p], want[p][0]) for p in range(n) if got_cells[p] != want[p][0]]
    assert not bad, ("score call", bad[:3])
    got = ctx.sw_align_banded(batch, sc, lo, hi, min_score)
    bad = [(p, lo[p], hi[p], got[p], want[p][1]) for p in range(n) if got[p] != ([want[p][1]] if want[p][1] else [])]
    assert not bad, ("align call", bad[:2])
    return want


def planted(rng, la, lb, diag, edits=0.08, alphabet=b"ACGT", keep=None):
    """seq_a of la letters, seq_b of lb letters: a stretch of seq_b, edited, is planted in seq_a so that it lies along the
    diagonal i - j = diag (as far as the pair's shape lets it); the rest is random."""
    b = bytes(rng.choice(alphabet) for _ in range(lb))
    j0 = max(0, -diag)
    i0 = j0 + diag
    n = max(0, min(la - i0, lb - j0, keep or lb))
    core = BL.mutate(rng, b[j0:j0 + n], edits, alphabet)
    a = bytes(rng.choice(alphabet) for _ in range(i0)) + core
    a = (a + bytes(rng.choice(alphabet) for _ in range(max(0, la - len(a)))))[:la]
    return a, b


# ---------------------------------------------------------------- 1. widths --
@pytest.mark.parametrize("width", WIDTHS)
def test_every_width_class_and_its_edges(ctx, width):
    """Three pairs per width: the hit along the band's left edge, along its right edge, and in the middle; the band right of
    the main diagonal, left of it and across it."""
    rng = random.Random(1000 + width)
    sc, osc = scoring(PLAIN)
    pairs, lo, hi = [], [], []
    for k, first in enumerate((7, -width - 5, -(width // 2))):
        lb = rng.randrange(130, 201)
        last = first + width - 1
        la = max(last, 0) + rng.randrange(40, 90)
        diag = (first, last, (first + last) // 2)[k]
        pairs.append(planted(rng, la, lb, diag))
        lo.append(first)
        hi.append(last)
        assert BS.width_of(la, lb, first, last) == min(last, la) - max(first, -lb) + 1
    assert BS.width_of(len(pairs[0][0]), len(pairs[0][1]), lo[0], hi[0]) == width     # pair 0's band is not clipped
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert sum(1 for cell, hit in want if hit) >= 2, want


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
    assert sum(1 for cell, hit in want if hit) >= 6, want


def test_bounds_far_outside_a_small_pair_are_the_unbanded_calls(ctx):
    rng = random.Random(77)
    sc, osc = scoring(PLAIN)
    pairs = [planted(rng, rng.randrange(1, 60), rng.randrange(1, 60), rng.randrange(-5, 6), 0.15) for _ in range(24)]
    batch = W.from_pairs(pairs)
    for lo, hi in ((-10 ** 6, 10 ** 6), (-2 ** 31, 2 ** 31 - 1)):
        check(ctx, sc, osc, pairs, lo, hi)
        got = ctx.sw_score_banded(batch, sc, lo, hi)
        full = ctx.sw_score(batch, sc)
        assert all(np.array_equal(g, f) for g, f in zip(got, full))
        assert ctx.sw_align_banded(batch, sc, lo, hi, 1) == ctx.sw_batch(batch, sc, 1, max_hits=1)


def test_empty_bands_and_empty_sequences(ctx):
    sc, osc = scoring(PLAIN)
    a, b = b"ACGTTGCAAGCTTGCA" * 3, b"GGACGTTGCAAGCTTGCATT" * 2
    la, lb = len(a), len(b)
    pairs = [(a, b), (a, b), (a, b), (a, b), (b"", b), (a, b""), (b"", b""), (a, b), (a, b)]
    lo = [la + 1, -lb - 9, la, -lb, -3, -3, 0, 2 ** 31 - 1, -2 ** 31]
    hi = [la + 70, -lb - 1, la, -lb, 3, 3, 0, 2 ** 31 - 1, -2 ** 31]
    want = check(ctx, sc, osc, pairs, lo, hi)
    assert all(cell == (0, 0, 0) and hit is None for cell, hit in want)
    # ... next to pairs that do have a hit
    mixed = [pairs[0], (a, b), pairs[4], (a, b), pairs[6]]
    want = check(ctx, sc, osc, mixed, [la + 1, -4, -3, -40, 0], [la + 70, 4, 3, 40, 0])
    assert [hit is not None for cell, hit in want] == [False, True, False, True, False]


def test_mixed_widths_in_one_batch_one_launch_per_class(ctx):
    rng = random.Random(5)
    sc, osc = scoring(PLAIN)
    widths = [1, 64, 65, 130, 300, 64, 700, 2, 1024, 513, 65]
    pairs, lo, hi = [], [], []
    for w in widths:
        first = rng.randrange(-40, 10)
        pairs.append(planted(rng, first + w + 60, rng.randrange(130, 180), first + w // 2))
        lo.append(first)
        hi.append(first + w - 1)
        assert BS.width_of(len(pairs[-1][0]), len(pairs[-1][1]), lo[-1], hi[-1]) == w
    check(ctx, sc, osc, pairs, lo, hi)
    classes = len({next(k for k, edge in enumerate(LADDER) if w <= edge) for w in widths})
    batch = W.from_pairs(pairs)
    ctx.sw_score_banded(batch, sc, lo, hi)
    assert ctx.last_call() == {"band_score": (classes, len(pairs))}
    ctx.sw_align_banded(batch, sc, lo, hi, 1)
    assert ctx.last_call() == {"band_fill": (classes, len(pairs)), "band_walk": (1, len(pairs))}


# ---------------------------------------------------------------- 3. planted ties of the maximum --
def two_segment_pair(rng, L, p, q, la, lb):
    """seq_a = A's with one C/G segment at each p (0-based start), seq_b = T's with the same segment at each q: the only
    matching letters are the segments', so the maximum 2 L stands at the end cell of every pair of copies on one diagonal."""
    seg = bytes(rng.choice(b"CG") for _ in range(L))
    a, b = bytearray(b"A" * la), bytearray(b"T" * lb)
    for x in p:
        a[x:x + L] = seg
    for y in q:
        b[y:y + L] = seg
    return bytes(a), bytes(b)


def assert_maxima(osc, a, b, lo, hi, cells):
    """On bandswlib alone: the banded maximum stands at exactly `cells` (column, row)."""
    M = BS.fill(osc, a, b, (lo, hi))[0].reshape(len(b) + 1, len(a) + 1)
    rows, cols = np.nonzero(M == M.max())
    assert sorted(zip(cols.tolist(), rows.tolist())) == sorted(cells), (sorted(zip(cols.tolist(), rows.tolist())), cells)


@pytest.mark.parametrize("lo,hi", [(-4, 4), (-60, 3), (-110, 20)])
def test_tie_with_a_column_that_has_left_the_frame(ctx, lo, hi):
    """(a) two equal segments on two diagonals of the band; by the row the higher column peaks, the lower one has left the
    frame.  The lower column is the hit."""
    rng = random.Random(31 - lo)
    sc, osc = scoring(PLAIN)
    L, p1, q1 = 20, 10, 10
    q2 = p1 + L - lo + 25                             # the frame's first column on row q2 + L is past p1 + L; 25 rows of
                                                      # mismatches in between take the first segment's score to 0
    p2 = q2 + hi - 1
    a, b = two_segment_pair(rng, L, (p1, p2), (q1, q2), p2 + L + 9, max(q2 + L + 6, 135))
    assert 130 <= len(b) <= 200
    assert q2 + L + lo > p1 + L
    assert_maxima(osc, a, b, lo, hi, [(p1 + L, q1 + L), (p2 + L, q2 + L)])
    want = check(ctx, sc, osc, [(a, b)], lo, hi)
    assert want[0][0] == (2 * L, p1 + L, q1 + L)


@pytest.mark.parametrize("gap", [14, 40])
def test_tie_in_one_column_two_rows(ctx, gap):
    """(b) one segment in seq_a, two in seq_b, both diagonals in the band: the column's position in the frame moves `gap`
    places between the two rows.  The lower row is the hit."""
    rng = random.Random(gap)
    sc, osc = scoring(PLAIN)
    L, p, q1 = 12, 90, 70
    q2 = q1 + gap
    lo, hi = p - q2 - 3, p - q1 + 3
    a, b = two_segment_pair(rng, L, (p,), (q1, q2), 160, 150)
    assert_maxima(osc, a, b, lo, hi, [(p + L, q1 + L), (p + L, q2 + L)])
    want = check(ctx, sc, osc, [(a, b)], lo, hi)
    assert want[0][0] == (2 * L, p + L, q1 + L)


@pytest.mark.parametrize("lo,hi,d2", [(-60, 3, -30), (-60, 3, 3), (-100, 27, -50)])
def test_tie_with_the_column_that_leaves_on_that_row(ctx, lo, hi, d2):
    """(c) the lower column leaves the frame through lane 0 on the very row the higher one peaks."""
    rng = random.Random(hi - lo + d2)
    sc, osc = scoring(PLAIN)
    L, p1, q1 = 20, 10, 10
    q2 = p1 + 1 - lo                                  # row q2 + L: the frame's first column becomes p1 + L + 1
    p2 = q2 + d2
    a, b = two_segment_pair(rng, L, (p1, p2), (q1, q2), max(p2 + L + 5, 60), q2 + L + 40)
    assert (q2 + L) + lo == (p1 + L) + 1 and 130 <= len(b) <= 200
    assert_maxima(osc, a, b, lo, hi, [(p1 + L, q1 + L), (p2 + L, q2 + L)])
    want = check(ctx, sc, osc, [(a, b)], lo, hi)
    assert want[0][0] == (2 * L, p1 + L, q1 + L)


# ---------------------------------------------------------------- 4. scorings --
def _protein():
    presets = json.loads((Path(__file__).resolve().parent / "golden" / "presets.json").read_text())
    sc = S.make_scoring({"preset": "BLOSUM62"})
    assert bytes(O.build_scoring(presets["BLOSUM62"]["spec"]))[:8] == bytes(sc)[:8]
    return sc, O.Scoring.from_buffer_copy(bytes(sc)), b"ARNDCQEGHILKMFPSTWYV"


SCORINGS = {
    "match_mismatch": lambda: (*scoring([1, -2, -4, -1]), b"ACGT"),
    "gap_extend_0": lambda: (*scoring([2, -3, -5, 0]), b"ACGT"),
    "gap_open_0": lambda: (*scoring([2, -3, 0, -2]), b"ACGT"),
    "blosum62": _protein,
    "wildcard": lambda: (*scoring([2, -3, -4, -1], wildcards=[["N", -1]]), b"ACGTN"),
    "case_sensitive": lambda: (*scoring([3, -2, -5, -2, 0, 0, 0, 0, 0, 1], mutations=[["a", "A", 1]]), b"ACGTacgt"),
    "no_start_no_end_gap": lambda: (*scoring([1, -2, -4, -1, 1, 1]), b"ACGT"),
    "no_gaps_in_a": lambda: (*scoring([2, -3, -4, -1, 0, 0, 1, 0]), b"ACGT"),
    "no_gaps_in_b": lambda: (*scoring([2, -3, -4, -1, 0, 0, 0, 1]), b"ACGT"),
    "no_mismatches": lambda: (*scoring([2, -3, -4, -1, 0, 0, 0, 0, 1]), b"ACGT"),
    "all_flags": lambda: (*scoring([2, -3, -4, -1, 1, 1, 1, 1, 1]), b"ACGT"),
    "gap_extend_plus_1": lambda: (*scoring([2, -3, -6, 1]), b"ACGT"),
}


@pytest.mark.parametrize("name", list(SCORINGS))
def test_scorings(ctx, name):
    """Per scoring eight pairs over four widths (one and several columns per lane), bands on both sides of the diagonal; with
    gap_extend = +1 the walk may leave the band and the definition decides: a cell outside reads 0."""
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
    assert sum(1 for cell, hit in want if hit) >= 6, want
    if name == "gap_extend_plus_1":
        left = [p for p, (cell, hit) in enumerate(want) if hit and not (lo[p] <= BS.hit_excursion(hit)[0] and BS.hit_excursion(hit)[1] <= hi[p])]
        assert left, "no walk left its band"


# ---------------------------------------------------------------- 5. errors, capacities, chunks --
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
    inside = W.from_pairs([good, good, (with_x, far), (with_x, near), good, (with_x, near)])
    for call, tail in ((ctx.sw_score_banded, ()), (ctx.sw_align_banded, (1,))):
        with pytest.raises(S.SeqAlignError) as got:
            call(inside, sc, -8, 8, *tail)
        assert got.value.code == S.E_UNKNOWN_PAIR and "pair 3:" in str(got.value), str(got.value)
    assert BS.fill_unknown(osc, with_x, near, (-8, 8))[3] == [(101, 104)]
    assert BS.fill_unknown(osc, with_x, far, (-8, 8))[3] == []
    want = check(ctx, sc, osc, [good, (with_x, far), good], -8, 8)
    assert all(hit for cell, hit in want)


def test_min_score_and_capacities(ctx):
    rng = random.Random(9)
    sc, osc = scoring(PLAIN)
    pairs = [planted(rng, 150, 140, d) for d in (0, 3, -4, 2, 0, -1)]
    want = check(ctx, sc, osc, pairs, -8, 8)
    scores = [cell[0] for cell, hit in want]
    assert all(s > 20 for s in scores)
    # min_score per pair: above the score, no hit; at the score, the hit
    ms = [scores[0] + 1, scores[1], 1, scores[3] + 50, -5, scores[5]]
    batch = W.from_pairs(pairs)
    got = ctx.sw_align_banded(batch, sc, -8, 8, ms)
    assert got == [[] if p in (0, 3) else [want[p][1]] for p in range(6)]
    # capacities: the hits that fit come first, in pair order, then E_NOMEM
    n = len(pairs)
    lo, hi, one = np.full(n, -8, np.int32), np.full(n, 8, np.int32), np.ones(n, np.int32)
    lens = [len(hit["a"]) for cell, hit in want]
    d = S.batch_desc(batch)

    def call(hit_cap, str_cap):
        hits, nh = (S.SwHit * n)(), C.c_uint64(99)
        oa, ob = np.zeros(max(1, str_cap), np.uint8), np.zeros(max(1, str_cap), np.uint8)
        rc = S.lib().seqalign_sw_align_banded(ctx._h, C.byref(d), C.byref(sc), S._ptr(lo), S._ptr(hi), S._ptr(one), hits,
                                              C.c_uint64(hit_cap), C.byref(nh), S._ptr(oa), S._ptr(ob), C.c_uint64(str_cap))
        out = [dict(score=h.score, pos_a=h.pos_a, pos_b=h.pos_b, len_a=h.len_a, len_b=h.len_b,
                    a=oa[h.str_off:h.str_off + h.length].tobytes().decode(), b=ob[h.str_off:h.str_off + h.length].tobytes().decode())
               for h in hits[:nh.value]]
        assert [h.pair for h in hits[:nh.value]] == list(range(nh.value))
        return rc, out

    full = sum(lens) + n
    assert call(n, full) == (0, [hit for cell, hit in want])
    assert call(4, full) == (S.E_NOMEM, [hit for cell, hit in want[:4]])
    assert call(n, lens[0] + lens[1] + 2 + lens[2]) == (S.E_NOMEM, [hit for cell, hit in want[:2]])
    assert call(0, full) == (S.E_NOMEM, [])
    assert call(n, 0) == (S.E_NOMEM, [])


def test_three_chunks_give_the_same_results(ctx):
    rng = random.Random(12)
    sc, osc = scoring(PLAIN)
    pairs = [planted(rng, 330, 200, rng.randrange(-20, 20)) for _ in range(6)]
    lo = [rng.randrange(-160, -120) for _ in pairs]
    hi = [rng.randrange(100, 140) for _ in pairs]
    want = check(ctx, sc, osc, pairs, lo, hi)
    batch = W.from_pairs(pairs)
    one = ctx.sw_align_banded(batch, sc, lo, hi, 1)
    assert ctx.last_call()["band_walk"] == (1, 6)
    with ctx.options(chunk_bytes=1 << 20):             # the smallest budget; a pair's align call needs ~12 x 200 x 260 bytes
        got = ctx.sw_align_banded(batch, sc, lo, hi, 1)
        info = ctx.last_call()
        assert info["band_walk"][0] >= 3 and info["band_walk"][1] == 6, info
        score = ctx.sw_score_banded(batch, sc, lo, hi)
        wide = W.from_pairs([pairs[0], planted(rng, 1100, 200, 5)])   # 12 x 200 x 1 000 bytes: pair 1 does not fit alone
        with pytest.raises(S.SeqAlignError) as e:
            ctx.sw_align_banded(wide, sc, -100, 899, 1)
        assert e.value.code == S.E_NOMEM and "pair 1:" in str(e.value) and "bytes" in str(e.value)
        assert int(ctx.sw_score_banded(wide, sc, -100, 899)[0][1]) == BS.expected(osc, *wide_pair(wide), -100, 899)[0][0]
    assert got == one == [[hit] for cell, hit in want]
    assert [int(s) for s in score[0]] == [cell[0] for cell, hit in want]


def test_time_hook_refuses_a_batch_of_several_chunks(ctx):
    """seqalign_sw_band_score_time_ms times the launches of ONE chunk: a batch of more than 1 MiB at chunk_bytes = 1 MiB is
    SEQALIGN_E_ARG with the hook's own message; at the default budget it returns `repeats` positive times."""
    sc, _ = scoring(PLAIN)
    batch = W.from_pairs([(b"ACGT" * 50, b"ACGTTACGTACGAT" * 14)] * 4000)   # 200 + 196 + 80 bytes per pair: 1.9 MB
    with ctx.options(chunk_bytes=1 << 20):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_band_score_time_ms(batch, sc, -10, 10, repeats=3)
    assert err.value.code == S.E_ARG and "seqalign_sw_band_score_time_ms: the batch does not fit one chunk" in str(err.value), str(err.value)
    ms = ctx.sw_band_score_time_ms(batch, sc, -10, 10, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms


def wide_pair(batch):
    return batch.seq_a(1), batch.seq_b(1)


# ---------------------------------------------------------------- 6. seeded random section --
def test_seeded_random_trials(ctx):
    """40 trials of at most 4 pairs of at most 260 x 260 under random scorings, flags and bounds."""
    rng = random.Random(20263)
    n_hits = n_pairs = 0
    for trial in range(40):
        flags = [int(rng.random() < 0.2) for _ in range(5)]
        ge = rng.choice([-1, -2, 0, -1, -3])
        init = [rng.choice([1, 2, 5]), rng.choice([-1, -3, -4]), rng.choice([0, -2, -4, -10]), ge, *flags, rng.randrange(2)]
        sc, osc = scoring(init)
        pairs, lo, hi = [], [], []
        for _ in range(rng.randrange(1, 5)):
            la, lb = rng.randrange(0, 261), rng.randrange(0, 261)
            diag = rng.randrange(-lb, la + 1)
            pairs.append(planted(rng, la, lb, diag, rng.choice([0.0, 0.1, 0.3]), b"ACGTacgt", keep=rng.randrange(10, 200)))
            first = diag - rng.randrange(0, 40) + rng.choice([0, 0, 0, 60, -300])
            lo.append(first)
            hi.append(first + rng.choice([0, 1, 5, 20, 63, 64, 100, 300, 520]))
        want = check(ctx, sc, osc, pairs, lo, hi, rng.choice([1, 1, 10, -3]))
        n_pairs += len(pairs)
        n_hits += sum(1 for cell, hit in want if hit)
    assert n_hits >= n_pairs // 3, (n_hits, n_pairs)
