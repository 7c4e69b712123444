"""CPU tier: the argument that tests/test_gpu_sw_span_dense.py and tests/test_gpu_band_dense.py test what they claim -- on the
oracle and the Python definitions alone (orclib, spanlib, bandswlib, bandlib), without a device.

The span kernel (sa_span.hip) finds sw_batch's first hit with device code of its own, and the banded and long calls
(sa_band.hip, sa_band_strips.hip, sa_align_long.hip) with theirs.  Three kinds of input tell a subtly wrong kernel from a right
one, and none of them reached these calls: pairs whose hit puts an insertion run directly against a deletion run (GAP_A
reached from GAP_B), pairs whose span depends on the walker's tie order, and the flags that change a row's recurrence --
each at every width class, across strip seams, and under bands that cut the alignment.  Every "at least" the GPU files rest
on is asserted here, with the measured figure printed beside it.
"""
import itertools

import pytest

import bandlib as BL
import bandswlib as BS
import denselib as D
import orclib as O
import seqalign_amd as S
import spanlib as SP
from seqalign_amd import workloads as W


def osc_of(spec):
    return O.Scoring.from_buffer_copy(bytes(S.make_scoring(spec)))


def first_hit(osc, a, b):
    rc, hits = O.oracle_sw(osc, a, b, 1, 1)
    assert rc == 0 and hits
    return hits[0]


def rows_class(len_a):
    """Columns per lane of the rows kernel that takes a pair (sa_launch_span_rows: 1 .. 6 and 8, one wave of 64 lanes)."""
    return min(c for c in (1, 2, 3, 4, 5, 6, 8) if 64 * c >= len_a)


def span_of(h):
    return (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"])


# ------------------------------------------------------------------------------------------- A1: gap-dense pairs, spans ---
# alternation's own hits cross a seam in at least half of the pairs of a cell (strips shape x scoring) except in these three,
# where the hit is short and sits at the right end of the row, or (ext0) most hits stay left of column 512: {cell: pairs of 8}
FEW_CROSSINGS = {("swdense", 700, 64): 0, ("ext0", 1100, 150): 3, ("ext0", 1600, 90): 3}


@pytest.mark.parametrize("scoring", D.SW_SCORINGS)
def test_span_dense_pairs_have_their_transitions_and_cross_the_seams(scoring):
    """Every counted pair (alternation, k = 0 .. 7) and every seam pair (straddling) of every span shape: at least 8 I->D in
    the first hit, no D->I.  Per strips shape: how many hits strictly contain a multiple of 512 in their column range -- at
    least half of alternation's pairs except in FEW_CROSSINGS's cells (pinned at their count), every straddling pair, so at
    least half of both together everywhere; every pair at 1 100 x 1 100.  spanlib.walk_both is the oracle's first hit."""
    osc = D.oracle_scoring(scoring)
    lowest = None
    for la, lb in D.SPAN_ROWS_SHAPES + D.SPAN_STRIPS_SHAPES:
        counted, seam = D.span_counted(la, lb, scoring), D.span_seam(la, lb, scoring)
        assert len(counted) == 8 and len(set(counted)) == 8 and len(seam) in (0, 8)
        hits = [first_hit(osc, a, b) for a, b in counted + seam]
        for (a, b), h in zip(counted + seam, hits):
            n_id = D.count_id(h["a"], h["b"])
            assert n_id >= 8 and D.count_di(h["a"], h["b"]) == 0, (scoring, la, lb, n_id)
            lowest = min(lowest or n_id, n_id)
        if la <= D.SPAN_STRIP_COLS:
            assert not seam
            continue
        across = [SP.crosses_seam(span_of(h)) for h in hits]
        alt, strad = sum(across[:8]), sum(across[8:])
        print(f"{scoring} {la}x{lb}: seam-crossing hits {alt} of 8 alternation, {strad} of {len(seam)} straddling")
        if (scoring, la, lb) in FEW_CROSSINGS:
            assert alt == FEW_CROSSINGS[(scoring, la, lb)] and seam
        else:
            assert 2 * alt >= 8, (scoring, la, lb, alt)
        assert strad == len(seam) and 2 * (alt + strad) >= 8 + len(seam)
        if (la, lb) == (1100, 1100):
            assert alt == 8 and all(h["pos_a"] < 512 and h["pos_a"] + h["len_a"] > 1024 for h in hits[:8])      # two seams
        if (la, lb) in ((577, 129), (1600, 700)):       # walk_both is the oracle's first hit
            for (a, b), h in zip(counted, hits):
                assert SP.walk_both(osc, a, b)[0] == span_of(h)
    print(f"{scoring}: the lowest I->D count of a counted pair is {lowest}")
    assert {la for la, _ in D.SPAN_ROWS_SHAPES[:-1]} == {60, 100, 130, 190, 250, 320, 384, 512}
    assert sorted({rows_class(la) for la, _ in D.SPAN_ROWS_SHAPES}) == [1, 2, 3, 4, 5, 6, 8]      # every class of the launcher


def test_span_dense_strips_pairs_are_tie_sensitive_under_ties():
    """Under [1,0,0,0] at least half of the counted pairs of the strips shapes give another span when the predecessor priority
    is reversed (M > B > A): a strips kernel with the wrong tie order cannot pass."""
    osc = D.oracle_scoring("ties")
    total = n = 0
    for la, lb in D.SPAN_STRIPS_SHAPES:
        both = [SP.walk_both(osc, a, b) for a, b in D.span_counted(la, lb, "ties")]
        sens = sum(w != r for w, r in both)
        print(f"ties {la}x{lb}: tie-sensitive {sens} of {len(both)}")
        total, n = total + sens, n + len(both)
    assert 2 * total >= n, (total, n)


def test_span_added_pairs_are_only_ever_added():
    for scoring in D.SW_SCORINGS:
        for la, lb in D.SPAN_ROWS_SHAPES + D.SPAN_STRIPS_SHAPES:
            added = D.span_added(la, lb, scoring)
            assert added and not set(added) & set(D.span_counted(la, lb, scoring) + D.span_seam(la, lb, scoring))
            assert all((len(a), len(b)) == (la, lb) for a, b in added)


# ------------------------------------------------------------------------------------------- A2: tie-dense pairs, spans ---
@pytest.mark.parametrize("name", list(SP.TIE_SCORINGS))
def test_tie_pairs_are_tie_sensitive_in_every_class_and_cross_the_seams(name):
    """40 pairs per (scoring, width): tie-sensitive at least 10 % under [2,-1,0,-1] and [3,-1,-1,0], at least 50 % under
    [2,-3,-2,1]; for the widths of several strips at least 25 % of all pairs have a hit that crosses a multiple of 512.  Every
    pair of a width lies in ONE class of the launcher."""
    osc = osc_of({"init": SP.TIE_SCORINGS[name] + [0] * 6})
    for width in SP.TIE_ROWS_WIDTHS + SP.TIE_STRIPS_WIDTHS:
        pairs = SP.tie_pairs(name, width)
        assert len(pairs) == 40 and all(1 <= len(b) <= 140 for a, b in pairs)
        if width <= 512:
            assert len({rows_class(len(a)) for a, b in pairs}) == 1 and all(len(a) <= 512 for a, b in pairs)
        else:
            assert len({-(-len(a) // 512) for a, b in pairs}) == 1 and all(len(a) > 512 for a, b in pairs)
        both = [SP.walk_both(osc, a, b) for a, b in pairs]
        sens, across = sum(w != r for w, r in both), sum(SP.crosses_seam(w) for w, r in both)
        print(f"{name} width {width}: tie_sensitive {sens} of 40, seam-crossing hits {across} of 40")
        assert sens >= (20 if name == "ext_pos" else 4), (name, width, sens)
        if width > 512:
            assert across >= 10, (name, width, across)
    # the walks are spanlib's own on small pairs, and the first of them is the oracle's hit
    small = SP.tie_pairs(name, 200)[:6]
    want = SP.want_spans(osc, W.from_pairs(small))
    for (a, b), w in zip(small, want):
        assert SP.walk_both(osc, a, b) == (SP.walk_span(osc, a, b), SP.walk_span(osc, a, b, SP.REVERSED)) and SP.walk_both(osc, a, b)[0] == w


@pytest.mark.parametrize("name", list(SP.SEAM_SCORINGS))
def test_seam_pairs_tell_the_tie_order_at_the_seam(name):
    """The tie-dense and gap-dense pairs above change their span when the priority is reversed everywhere, but not one of
    them when it is lost on the steps across a seam only (asserted below on the widest tie cell): the kernel's `zwins` and
    `out.from_a` could be wrong unnoticed.  seam_pairs: at least half of the 24 pairs per width (ext_pos: a quarter) change
    their span when gap_b wins the tie with gap_a on the DIAGONAL step across a seam, at every seam of the width.  On the
    horizontal step no pair can: where the opening from gap_a ties with the extension of gap_b, the two gaps taken in the
    other order score the same, gap_a of the cell the walk arrives in ties too, and the walker leaves upwards (0 recorded)."""
    osc = osc_of({"init": SP.SEAM_SCORINGS[name] + [0] * 6})
    for width in SP.SEAM_WIDTHS[name]:
        pairs = SP.seam_pairs(name, width)
        assert len(pairs) == SP.SEAM_N and len({-(-len(a) // 512) for a, b in pairs}) == 1 and all(len(a) > 512 and 1 <= len(b) <= 140 for a, b in pairs)
        walks = [SP.walk_seams(osc, a, b) for a, b in pairs]
        diag, horiz = [w[0] != w[1] for w in walks], sum(w[0] != w[2] for w in walks)
        print(f"{name} width {width}: {sum(diag)} of {len(pairs)} spans change with the tie order lost at a seam (diagonal step), {horiz} (horizontal)")
        assert sum(diag) >= (len(pairs) // 4 if name == "ext_pos" else len(pairs) // 2) and horiz == 0
        if name != "ext_pos":       # every seam of the width is the one a telling pair's hit crosses
            seams = {s for w, d in zip(walks, diag) if d for s in range(512, width, 512) if SP.crosses_seam(w[0]) and w[0][1] < s < w[0][1] + w[0][3]}
            assert seams == set(range(512, width, 512)), (name, width, seams)
        for (a, b), w in list(zip(pairs, walks))[:4]:
            assert [w[0]] == SP.want_spans(osc, W.from_pairs([(a, b)]))
    if name in SP.TIE_SCORINGS:
        assert all(len(set(SP.walk_seams(osc, a, b))) == 1 for a, b in SP.tie_pairs(name, 1600))


# -------------------------------------------------------------------------------------------------- A3: flags, wide rows ---
def flag_spans(flags):
    osc = osc_of(SP.flag_spec(*flags))
    return [s for width in SP.FLAG_WIDTHS for s in SP.want_spans(osc, W.from_pairs(SP.flag_pairs(width)))]


def test_flags_change_the_spans_of_the_wide_pairs():
    """Each of the 7 non-zero combinations of no_gaps_in_a, no_gaps_in_b and no_mismatches changes the span of at least 5 of
    the 20 pairs; no_start_gap_penalty and no_end_gap_penalty change none (a free end gap lies in the last column or row, and
    no match cell follows it) -- the pairs: a hit that reaches the last column, one that ends on the last row, and more."""
    plain = flag_spans((0, 0, 0))
    assert len(plain) == 20 and all(s[0] > 0 for s in plain)
    per_width = [plain[4 * k:4 * k + 4] for k in range(5)]
    for width, (last_col, last_row, middle, _) in zip(SP.FLAG_WIDTHS, per_width):
        assert last_col[1] + last_col[3] == width and last_col[3] > 20                       # reaches the last column
        assert last_row[2] + last_row[4] == len(SP.flag_pairs(width)[1][1]) and last_row[1] < 64     # ends on the last row
        assert width // 2 - 60 < middle[1] < width // 2 + 60
    for flags in itertools.product([0, 1], repeat=3):
        if any(flags):
            differ = sum(x != y for x, y in zip(flag_spans(flags), plain))
            print(f"no_gaps_in_a, no_gaps_in_b, no_mismatches = {flags}: {differ} of 20 spans differ")
            assert differ >= 5, (flags, differ)
    for ends in ((0, 1), (1, 0), (1, 1)):
        assert flag_spans((0, 0, 0, *ends)) == plain, ends


# --------------------------------------------------------------------------------------- B1: bands on gap-dense pairs ---
SQUARE = tuple(s for s in D.BAND_SHAPES if s[0] == s[1])


@pytest.mark.parametrize("scoring", D.SW_SCORINGS)
def test_a_band_turns_the_transitions_round(scoring):
    """alternation pairs under a band.  (0, +1) is the unbanded hit's excursion: at least 8 I->D.  (-1, 0) is its mirror: at
    least 8 D->I -- a move order alignment_reverse_move never produces without a band.  On the square shapes the two are
    exact mirrors: the same score, not one transition of the other kind.  (0, 0): no gap column at all.  The whole-matrix
    band is the oracle's first hit."""
    osc = D.oracle_scoring(scoring)
    assert SQUARE == ((150, 150), (500, 500))
    for la, lb in D.BAND_SHAPES:
        low_id = low_di = None
        for a, b in D.band_pairs(la, lb, scoring):
            assert D.sw_bands(la, lb)[2:5] == [(0, 1), (-1, 0), (0, 0)]
            (up_cell, up), (down_cell, down), (diag_cell, diag) = (BS.expected(osc, a, b, lo, hi) for lo, hi in D.sw_bands(la, lb)[2:5])
            n_id, n_di = D.count_id(up["a"], up["b"]), D.count_di(down["a"], down["b"])
            assert n_id >= 8 and n_di >= 8, (scoring, la, lb, n_id, n_di)
            assert BS.hit_excursion(up) == (0, 1) and BS.hit_excursion(down) == (-1, 0)
            if (la, lb) in SQUARE:
                assert up["score"] == down["score"] and n_id == n_di
                assert D.count_di(up["a"], up["b"]) == 0 and D.count_id(down["a"], down["b"]) == 0
            assert "-" not in diag["a"] + diag["b"] and diag["score"] <= up["score"]
            low_id, low_di = min(low_id or n_id, n_id), min(low_di or n_di, n_di)
            whole = BS.expected(osc, a, b, -lb, la)
            h = first_hit(osc, a, b)
            assert whole[1] == h and whole[0] == (h["score"], h["pos_a"] + h["len_a"], h["pos_b"] + h["len_b"])
        print(f"{scoring} {la}x{lb}: at least {low_id} I->D under (0, 1), at least {low_di} D->I under (-1, 0)")
    if scoring == "swdense":      # the figures the cases were chosen by
        a, b = D.alternation(150, 150, 3)
        up, down, diag = (BS.expected(osc, a, b, lo, hi)[1] for lo, hi in ((0, 1), (-1, 0), (0, 0)))
        assert (up["score"], down["score"], D.count_id(up["a"], up["b"]), D.count_di(down["a"], down["b"])) == (239, 239, 73, 73)
        assert (diag["score"], len(diag["a"])) == (20, 4)


def transition_columns(hit, kind):
    """The column of seq_a (mod 64; 0 is a strip's last column, 1 its first) of the I step of each transition of the kind
    ("ID" or "DI")."""
    ops, col, at = D.ops(hit["a"], hit["b"]), hit["pos_a"], set()
    for c in range(len(ops)):
        col += ops[c] != "D"
        if ops[c:c + 2] == kind:
            at.add((col + (kind == "DI")) % 64)
    return at


@pytest.mark.parametrize("scoring", D.SW_SCORINGS)
def test_the_band_cases_put_transitions_in_every_column_of_a_strip(scoring):
    """The wide calls run with band_strip_cols = 64.  alternation's period is two columns of seq_a (three steps), so its
    transitions stand in every second column only -- on one side of every strip seam, never the other.  The two spaced pairs added
    at 500 x 500 shift them: I->D under (0, 1) and D->I under (-1, 0) in every one of a strip's 64 columns (ext0, whose period
    is four columns: at least 60)."""
    osc = D.oracle_scoring(scoring)
    for (lo, hi), kind in (((0, 1), "ID"), ((-1, 0), "DI")):
        alt = set().union(*(transition_columns(BS.expected(osc, a, b, lo, hi)[1], kind) for a, b in D.band_pairs(500, 500, scoring)))
        if D.matches_of(scoring) == 1:
            assert len(alt) == 32 and len({c % 2 for c in alt}) == 1, (kind, sorted(alt))
        hits = [BS.expected(osc, a, b, lo, hi)[1] for a, b in D.band_added(500, 500, scoring)]
        assert all(h["a"].count("-") >= 60 for h in hits)
        at = set().union(*(transition_columns(h, kind) for h in hits))
        print(f"{scoring} ({lo}, {hi}): {kind} in {len(at)} of a strip's 64 columns")
        assert len(at) >= (60 if scoring == "ext0" else 64) and {0, 1} <= at, (kind, sorted(set(range(64)) - at))


NW_OF = {"swdense": "cheap0", "ties": "ties", "ext0": "ext0"}


@pytest.mark.parametrize("scoring", D.SW_SCORINGS)
def test_nw_bands_on_the_band_pairs(scoring):
    """The wide NW calls run the band pairs under bands 0, 1, 3 and 40: every pair has an alignment inside each; bands 3 and 40
    hold the unbanded alignment (the banded result is the oracle's), band 0 cuts it for most pairs."""
    osc = D.oracle_scoring(NW_OF[scoring])
    cut = n = 0
    for la, lb in D.BAND_SHAPES:
        for a, b in D.band_pairs(la, lb, scoring) + D.band_added(la, lb, scoring):
            full = O.oracle_nw(osc, a, b)[1:]
            assert D.count_id(*full[1:]) >= 8
            want = [BL.expected(osc, a, b, w) for w in (0, 1, 3, 40)]
            assert all(x is not None for x in want) and want[2] == want[3] == full
            cut, n = cut + (want[0] != full), n + 1
    print(f"{scoring}: band 0 cuts the alignment of {cut} of {n} pairs")
    assert 2 * cut >= n


def test_the_pair_past_the_narrow_cap():
    """alternation(1 300, 1 300): 1 201 diagonals under (-600, 600) and under NW's band 600 -- past the narrow calls' 1 024 --
    and dense all the way."""
    la, lb = D.PAST_CAP["shape"]
    a, b = D.alternation(la, lb)
    name, lo, hi = D.PAST_CAP["sw"]
    assert BS.width_of(la, lb, lo, hi) == 1201 > 1024
    cell, hit = BS.expected(D.oracle_scoring(name), a, b, lo, hi)
    assert D.count_id(hit["a"], hit["b"]) >= 600 and cell[0] == hit["score"]
    name, w = D.PAST_CAP["nw"]
    assert BL.width_of(la, lb, w) == 1201
    score, ra, rb = BL.expected(D.oracle_scoring(name), a, b, w)
    assert D.count_id(ra, rb) >= 600 and D.count_di(ra, rb) == 0
    assert (score, ra, rb) == O.oracle_nw(D.oracle_scoring(name), a, b)[1:]


def test_the_long_sw_pairs_are_dense():
    """sw_align_long's pairs: under swdense and ties every alternation and spaced pair's first hit at min_score SW_MIN_SCORE
    has I->D transitions (the two long-runs pairs have their one), the 1 100 x 300 pair over 140 of them."""
    for scoring in ("swdense", "ties"):
        pairs = D.long_sw_pairs()
        assert pairs[-1] == D.alternation(1100, 300) and len(pairs) == 9
        counts = []
        for a, b in pairs:
            rc, hits = O.oracle_sw(D.oracle_scoring(scoring), a, b, D.SW_MIN_SCORE, 1)
            assert rc == 0 and hits
            counts.append(D.count_id(hits[0]["a"], hits[0]["b"]))
        print(f"{scoring}: I->D per pair {counts}")
        assert all(c >= 8 for c in counts[:5]) and counts[5] >= 3 and counts[-1] >= 140 and sum(c >= 1 for c in counts) >= 7, counts
