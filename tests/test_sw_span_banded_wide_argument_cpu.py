"""CPU tier: what seqalign_sw_span_banded_wide's kernel rests on, checked against the oracle without a device.

The kernel's schedule over two full-word payloads (bandspanwidelib.strip_model: the strips and their rows, the standing and the
moving frame, the stop feed and the hand-off entries, the up-left of a strip's first row, the reset above the right edge, the
retire, the end pick per strip and the merge of the left strip's best entry) gives the five values of the oracle's banded hit
(bandspanlib.want) at strips of 1, 2, 3, 7 and 64 columns, under all 32 flag combinations, the three tie scorings (one of which
has a gap extension that pays) and a plain scoring; no band cell reads a frame position, a hand-off entry or a best entry that
holds no band cell's values (the model carries POISON there and asserts).  The tests assert their own coverage, so that inputs
that miss a case fail here."""
import itertools

import pytest

import bandspanlib as BSP
import bandspanwidelib as BW
import spanlib as SP
from test_sw_span_argument_cpu import oracle_scoring

STRIPS = (1, 2, 3, 7, 64)
N_PAIRS, N_LONG, N_FLAG_PAIRS, N_FLAG_LONG = 120, 60, 24, 10
# spanlib.TIE_SCORINGS over a binary alphabet (ext_pos: the gap extension pays), and the plain scoring of the narrow call's tests
SCORINGS = {**{name: (init, b"AC") for name, init in SP.TIE_SCORINGS.items()}, "plain": ([2, -3, -4, -1], b"ACGT")}
COUNTED = ("late_start", "both_phases", "entries", "stop_feeds", "tie_left", "tie_retired")
SEED = 4300


def pairs_of(seed, n_small, n_long, alpha):
    return BSP.band_pairs(seed, n_small, alpha, max_width=14) + BW.long_band_pairs(seed + 1, n_long, alpha)


def new_total():
    return dict({key: 0 for key in COUNTED}, kinds=set(), outside_left_of_seam=0, multi_busy=0)


def models_and_want(osc, a, b, lo, hi, total):
    """The wanted five after checking that the model gives them at every strip width; adds the coverage of every run to
    `total`."""
    want = BSP.want(osc, a, b, lo, hi)[1]
    la, lb = len(a), len(b)
    mats = BSP.banded_mats(osc, a, b, lo, hi) if BW.band_kind(la, lb, lo, hi) != "empty" and la and lb else None
    total["kinds"].add(BW.band_kind(la, lb, lo, hi))
    for S in STRIPS:
        got, cover = BW.strip_model(osc, a, b, lo, hi, S, mats)
        assert got == want, (S, a, b, lo, hi, got, want)
        assert cover["strips"] == max(1, -(-la // S))
        for key in COUNTED:
            total[key] += cover[key]
        total["multi_busy"] += cover["busy"] > 1
        total["outside_left_of_seam"] += BW.outside_left_of_seam(want, la, lb, lo, hi, S)
    return want


def assert_covered(total, gap_pays):
    assert total["kinds"] == {"empty", "left", "right", "mid"}, total      # bands wholly left, wholly right, across, and empty
    assert total["late_start"] > 0, total                                  # a strip whose first row is late
    assert total["both_phases"] > 0, total                                 # a strip that stands and then moves
    assert total["entries"] > 0 and total["stop_feeds"] > 0 and total["multi_busy"] > 0, total
    assert total["tie_left"] > 0, total                                    # a best cell tied between two strips: the left one wins
    assert total["tie_retired"] > 0, total                                 # a best cell tied between a retired and a live column
    if gap_pays:
        assert total["outside_left_of_seam"] > 0, total                    # a hit that starts outside the band, left of a seam
    else:
        assert total["outside_left_of_seam"] == 0, total


@pytest.mark.parametrize("name", list(SCORINGS))
def test_strip_schedule_equals_the_oracle(name):
    init, alpha = SCORINGS[name]
    osc = oracle_scoring({"init": [*init, 0, 0, 0, 0, 0, 0]})
    total = new_total()
    hits = sensitive_across_a_seam = 0
    for a, b, lo, hi in pairs_of(SEED + len(name), N_PAIRS, N_LONG, alpha):
        want = models_and_want(osc, a, b, lo, hi, total)
        hits += want[0] > 0
        if name in SP.TIE_SCORINGS and BW.crosses_seam(want, 7) and BSP.reversed_differs(osc, a, b, lo, hi):
            sensitive_across_a_seam += 1
    print(name, total, "hits", hits, "tie-sensitive across a seam at S = 7", sensitive_across_a_seam)
    assert hits >= (N_PAIRS + N_LONG) // 3, hits
    assert_covered(total, osc.gap_extend > 0)
    if name in SP.TIE_SCORINGS:                               # the tie rule is exercised across a seam
        assert sensitive_across_a_seam >= 1


def test_strip_schedule_under_all_flag_combinations():
    total = new_total()
    hits = pairs = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = oracle_scoring(spec)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        for a, b, lo, hi in pairs_of(5300 + idx, N_FLAG_PAIRS, N_FLAG_LONG, alpha):
            want = models_and_want(osc, a, b, lo, hi, total)
            pairs += 1
            hits += want[0] > 0
    print("pairs", pairs, "hits", hits, total)
    assert hits >= pairs // 3, (hits, pairs)
    assert total["kinds"] == {"empty", "left", "right", "mid"} and total["late_start"] and total["both_phases"] and total["entries"], total
