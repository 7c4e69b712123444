"""CPU tier: what the seqalign_nw_gaps_* kernels rest on, checked against the oracle without a device.

1. The numbers of '-' runs in the two strings of the alignment orclib.oracle_nw returns (nwgaplib.want_gaps) are a function of
   the three NW matrices alone and can be carried FORWARD beside them: nwgaplib.forward, the definition -- the border's own run,
   and a gap state adds one unless the predecessor the walker picks is the same gap state in a cell off the border -- equals a
   step-by-step walk and the counted strings.
2. The sweep's shape with every feed and hand-off RAW and the increment decided in the consuming cell (nwgaplib.kernel_model,
   strips of 5 to 7 columns) equals the definition state by state.  Under five scorings with the 32 flag combinations, the
   forbidding scorings, statlib.tie_pairs and denselib's families.
3. The same with bands (nwgaplib.frame_model) against the oracle's walk over the banded matrices, state by state: bands on,
   beside and off the alignment, and bands with no alignment inside (the mark).
4. The inputs bite, on the oracle alone: counts that change under the reversed priority, alignments that begin with a border
   run, runs in both strings -- and a model that puts (0, 0) on the whole border is wrong on EVERY pair that begins with a gap.
"""
import itertools

import pytest

import bandlib as BL
import bandnwstatlib as BN
import denselib as D
import nwgaplib as NG
import orclib as O
import statlib as ST
from seqalign_amd import workloads as W
from test_nw_stats_argument_cpu import FORBIDDING, forbidding_pairs, small_pairs

INITS = {"dna": [1, -2, -4, -1], "open0": [2, -1, 0, -1], "ext0": [3, -1, -1, 0], "ties": [1, 0, 0, 0], "ext_pos": [2, -3, -2, 1]}
FLAGS = list(itertools.product([0, 1], repeat=5))


def osc_of(spec):
    return O.build_scoring(spec, "oracle")


def check_pair(osc, a, b, want, strips=(1 << 30, 5, 6)):
    """definition == walk == kernel shape (state by state) == the '-' runs of the oracle's strings (None: its traceback fails).
    Returns whether the alignment begins with a border run; where it does, the flat-border model must be wrong."""
    expect = NG.NO_WALK if want is None else want
    res, run = NG.forward(osc, a, b)
    assert res == expect, ("forward", a, b, res, expect)
    walked, border = NG.walk(osc, a, b)
    assert walked == expect, ("walk", a, b, walked, expect)
    for strip in strips:
        assert NG.kernel_model(osc, a, b, strip, run) == expect, ("kernel model", strip, a, b)
    if want is not None and a and b:
        assert border == NG.begins_with_gap(osc, a, b)
        flat = NG.forward(osc, a, b, flat_border=True)[0]
        assert (flat != expect) == border, ("flat border", a, b, flat, expect)
    return border


@pytest.mark.parametrize("name", list(INITS))
def test_five_scorings_under_the_32_flag_combinations(name):
    """Lengths 0 to 14 over AC: short enough that most alignments touch the border away from the corner."""
    rng = W.Rng(1200 + len(name))
    n = both = border = 0
    for flags in FLAGS:
        osc = osc_of({"init": [*INITS[name], *flags, 0]})
        pairs = []
        for _ in range(6):
            la, lb = (int(x) for x in rng.below(15, 2))
            pairs.append((bytes(b"AC"[i] for i in rng.below(2, la)), bytes(b"AC"[i] for i in rng.below(2, lb))))
        for (a, b), w in zip(pairs, NG.want_gaps(osc, pairs)):
            assert w is not None
            border += check_pair(osc, a, b, w, strips=(1 << 30, 5, 7))
            n += 1
            both += w[1] > 0 and w[2] > 0
    assert 3 * both >= n and border >= n // 3, (n, both, border)


def test_mixed_case_wildcards_and_mutations():
    gapped = 0
    for idx, flags in enumerate(FLAGS):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        ext = 1 if idx % 5 == 2 else -1                     # some with a gap_extend that pays
        spec = {"init": [1, mismatch, -4 if ext < 0 else -2, ext, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        osc = osc_of(spec)
        batch = W.ragged(8, seed=900 + idx, max_len=30, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        pairs = [(batch.seq_a(p), batch.seq_b(p)) for p in range(batch.n_pairs)]
        for (a, b), w in zip(pairs, NG.want_gaps(osc, pairs)):
            assert w is not None
            check_pair(osc, a, b, w, strips=(1 << 30, 7))
            gapped += w[1] > 0 and w[2] > 0
    assert gapped >= 64, gapped


@pytest.mark.parametrize("flags", FORBIDDING, ids=lambda f: "+".join(sorted(f)))
@pytest.mark.parametrize("init4", [[1, -2, -4, -1], [1, 0, 0, 0], [2, -3, -2, 1]], ids=["dna", "ties", "ext_pos"])
def test_forbidding_scorings(flags, init4):
    """no_mismatches with no_gaps_in_a, no_gaps_in_b and both: over whole matrices every pair keeps an alignment (DESIGN.md
    3.21), most of them through the border; the marks of the states that have no walk agree state by state."""
    osc = osc_of(ST.init_spec(init4, **flags))
    pairs = forbidding_pairs(77 + len(flags) + init4[0], flags)
    border = 0
    for (a, b), w in zip(pairs, NG.want_gaps(osc, pairs)):
        assert w is not None
        border += check_pair(osc, a, b, w, strips=(1 << 30, 6))
    assert border >= 6, border


@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_tie_pairs_state_by_state(name):
    """statlib.tie_pairs at the narrowest width: the model equals the definition state by state, strips of 7 and 64 columns."""
    osc = osc_of(ST.init_spec(ST.TIE_SCORINGS[name]))
    pairs = ST.tie_pairs(name, ST.TIE_WIDTHS[0])[:8]
    for (a, b), w in zip(pairs, NG.want_gaps(osc, pairs)):
        check_pair(osc, a, b, w, strips=(7, 64))


@pytest.mark.parametrize("scoring", D.NW_SCORINGS)
def test_gap_dense_families(scoring):
    """denselib's shapes at their smallest: an insertion directly against a deletion is two runs, one in each string."""
    osc = D.oracle_scoring(scoring)
    pairs = [D.alternation(31, 40, k, D.matches_of(scoring)) for k in range(3)] + [D.spaced(31, 40, 7 + k, k) for k in range(3)] \
        + [D.staircase(31, 40)]
    adjacent = 0
    for (a, b), w in zip(pairs, NG.want_gaps(osc, pairs)):
        check_pair(osc, a, b, w, strips=(1 << 30, 6))
        rc, _, ra, rb = O.oracle_nw(osc, a, b)
        adjacent += D.count_id(ra, rb) + D.count_di(ra, rb) > 0
    assert adjacent >= 1, adjacent


# What the oracle gives on statlib.tie_pairs(name, width), 40 pairs each (DESIGN.md 3.34 holds the table): pairs whose run counts
# change under the REVERSED priority / that begin with a border run / that have a run in each string.
#   ext0     64: 13 /  6 / 33    200: 27 / 12 / 38    512: 39 /  9 / 40    700: 39 / 10 / 40    1100: 40 /  6 / 40
#   ties     64: 34 /  8 / 39    200: 40 / 14 / 38    512: 40 /  9 / 39    700: 40 / 11 / 40    1100: 40 /  7 / 40
#   ext_pos  every width: 0 / 40 / 40
# Every width meets every condition with the default seeds, so none is reseeded or dropped.
@pytest.mark.parametrize("width", ST.TIE_WIDTHS)
@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_the_tie_pairs_bite(name, width):
    osc = osc_of(ST.init_spec(ST.TIE_SCORINGS[name]))
    pairs = ST.tie_pairs(name, width)
    reversed_differs = border = both = 0
    for (a, b), w in zip(pairs, NG.want_gaps(osc, pairs)):
        mats = ST.matrices(osc, a, b, as_lists=False)
        walked, br = NG.walk(osc, a, b, mats=mats)
        assert walked == w and br == NG.begins_with_gap(osc, a, b)
        reversed_differs += NG.walk(osc, a, b, NG.REVERSED, mats)[0] != w
        border += br
        both += w[1] > 0 and w[2] > 0
    if name == "ext_pos":
        assert border == 40, border
    else:
        assert reversed_differs >= 10 and border >= 6, (reversed_differs, border)
    assert both >= 30, both


# ----------------------------------------------------------------------------------------------------------- bands ---
def check_band(osc, a, b, w, F=8):
    """The oracle's walk over the banded matrices == the definition over them == the frame model, state by state; None where
    no alignment lies inside the band."""
    want = NG.band_want(osc, a, b, w)
    expect = NG.NO_WALK if want is None else want
    band = BL.band_of(len(a), len(b), w)
    mats = tuple(X.tolist() for X in BL.fill(osc, a, b, band))
    res, run = NG.forward(osc, a, b, mats=mats, band=band)
    assert res == expect, ("forward", a, b, w, res, expect)
    got, phases = NG.frame_model(osc, a, b, w, F, run)
    assert got == expect, ("frame model", a, b, w, got, expect)
    return want, phases


@pytest.mark.parametrize("name", list(INITS))
def test_band_frame_under_the_32_flag_combinations(name):
    n = none = gapped = 0
    phases = set()
    for idx, flags in enumerate(FLAGS):
        osc = osc_of({"init": [*INITS[name], *flags, 0]})
        for a, b, w in BN.small_pairs(5100 + 40 * len(name) + idx, 6, b"AC"):
            want, ph = check_band(osc, a, b, w)
            phases |= ph
            n += 1
            none += want is None
            gapped += want is not None and want[1] + want[2] > 0
    assert phases == {NG.BORDER, NG.STOPPED, NG.MOVING} and none >= 1 and gapped >= n // 3, (phases, n, none, gapped)


@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_band_frame_on_tie_pairs_on_beside_and_off_the_alignment(name):
    """Per pair: the smallest band that holds the unbanded alignment (the results are the unbanded call's), half of it (the
    band cuts the alignment) and a band of the fewest diagonals the lengths allow."""
    osc = osc_of(ST.init_spec(ST.TIE_SCORINGS[name]))
    pairs = ST.tie_pairs(name, ST.TIE_WIDTHS[0])[:6]
    cut = 0
    for (a, b), unbanded in zip(pairs, NG.want_gaps(osc, pairs)):
        rc, _, ra, rb = O.oracle_nw(osc, a, b)
        need = BL.smallest_band(ra, rb, len(a), len(b))
        on, _ = check_band(osc, a, b, need, F=192)
        assert on == unbanded, (a, b, need, on, unbanded)
        for w in (need // 2, 0):
            beside, _ = check_band(osc, a, b, w, F=192)
            cut += beside != unbanded
    assert cut >= 4, cut


@pytest.mark.parametrize("flags", FORBIDDING, ids=lambda f: "+".join(sorted(f)))
def test_bands_with_no_alignment_inside(flags):
    """Forbidding scorings inside narrow bands: the pairs whose letters do not line up lose their alignment, the definition and
    the frame model carry the mark to the end pick exactly where the oracle's walk over the banded matrices fails."""
    mismatch = -6 if len(flags) == 3 else -2
    osc = osc_of(ST.init_spec([1, mismatch, -4, -1], **flags))
    none = kept = 0
    for a, b in forbidding_pairs(91 + len(flags), flags):
        for w in (0, 2):
            if BL.width_of(len(a), len(b), w) > 16:
                continue
            want, _ = check_band(osc, a, b, w, F=16)
            none += want is None
            kept += want is not None
    assert none >= 5 and kept >= 5, (none, kept)


def test_constructed_pair_holds_on_the_oracle_at_a_small_size():
    """nwgaplib.deleted_inserted at 400 letters: one run in each string."""
    a, b = NG.deleted_inserted(W.Rng(5), 400, 100, 40, 300, 25)
    (w,) = NG.want_gaps(osc_of(ST.init_spec(NG.BLOCK_INIT)), [(a, b)])
    assert w[1:] == (1, 1) and len(b) == 385, w
