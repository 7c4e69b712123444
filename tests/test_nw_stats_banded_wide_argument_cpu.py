"""CPU tier: what seqalign_nw_stats_banded_wide's kernel rests on, checked against the oracle without a device.

The kernel's schedule over payloads (bandnwstatwidelib.strip_model: the strips and their rows, the standing and the moving frame,
the three feeds, the up-left of a strip's first row, the reset of V and D above the right edge, the hand-off entries, the end pick
in the last strip) gives the banded end value and the counted columns of the oracle's walk over the banded matrices
(bandnwstatlib.want) at strips of 1, 2, 3, 7 and 64 columns, under all 32 flag combinations, the three tie scorings and a gap that
pays; the mark agrees with the value; no band cell reads a frame position or a hand-off entry that holds no band cell (the model
carries POISON there and asserts).  The test asserts its own coverage, so that inputs that miss a case fail here."""
import itertools

import pytest

import bandlib as BL
import bandnwstatlib as BN
import bandnwstatwidelib as BW
import bandspanlib as BSP
import orclib as O
import statlib as ST

STRIPS = (1, 2, 3, 7, 64)
N_PAIRS, N_LONG, N_FLAG_PAIRS, N_FLAG_LONG = 120, 40, 30, 10
SCORINGS = {**{name: (init, b"AC") for name, init in ST.TIE_SCORINGS.items()}, "extend_pays": ([3, -4, -9, 1], b"ACGT")}


def osc_of(spec):
    return O.build_scoring(spec, "oracle")


def pairs_of(seed, n_small, n_long, alpha):
    return BN.small_pairs(seed, n_small, alpha, max_width=12) + BW.long_pairs(seed + 1, n_long, alpha)


def models_and_want(osc, a, b, w, total):
    """The wanted three (None by the oracle's WALK, which at these small numbers is also the value's rule) after checking that the model gives them at every strip width; adds the coverage of
    every run to `total`."""
    both = BN.want_walked(osc, a, b, w)
    want = None if both is None else both[0]
    mats = tuple(X.tolist() for X in BL.fill(osc, a, b, BL.band_of(len(a), len(b), w)))
    for S in STRIPS:
        got, mark, cover = BW.strip_model(osc, a, b, w, S, mats)
        assert mark == (got[0] < BN.HALF) == (want is None), (S, a, b, w, got, mark, want)
        assert mark or got == want, (S, a, b, w, got, want)
        if len(a):
            assert cover["strips"] == -(-len(a) // S)
        total["feeds0"] |= cover["feeds0"]
        for key in ("late_start", "both_phases", "marked", "from_a", "entries"):
            total[key] += cover[key]
    return want, (both[1] if both else None)


def new_total():
    return dict(feeds0=set(), late_start=0, both_phases=0, marked=0, from_a=0, entries=0)


def assert_covered(total):
    assert total["feeds0"] == {BW.BORDER, BW.NOTHING, BW.MOVING}, total       # the three feed phases of strip 0
    assert total["late_start"] > 0, total                                     # a strip s > 0 starts at jf > 1
    assert total["both_phases"] > 0, total                                    # a strip s > 0 stands, then moves
    assert total["entries"] > 0 and total["marked"] > 0, total                # a hand-off entry carries the mark
    assert total["from_a"] > 0, total                                         # a hand-off entry carries from_a


@pytest.mark.parametrize("name", list(SCORINGS))
def test_strip_schedule_equals_the_oracle(name):
    init, alpha = SCORINGS[name]
    osc = osc_of(ST.init_spec(init))
    total = new_total()
    shorter = longer = three_strips = sensitive_across_a_seam = 0
    for a, b, w in pairs_of(1900 + len(name), N_PAIRS, N_LONG, alpha):
        want, walked = models_and_want(osc, a, b, w, total)
        assert want is not None, (name, a, b, w)             # a plain scoring loses no pair
        if len(a) >= 15:
            three_strips += 1
            shorter += len(a) < len(b)
            longer += len(a) > len(b)
        if name in ST.TIE_SCORINGS and BW.walk_crosses_seam(walked[1], walked[2], len(a), 7) and BN.counts_reversed_differ(osc, a, b, w):
            sensitive_across_a_seam += 1
    print(name, total, three_strips, shorter, longer, sensitive_across_a_seam)
    assert_covered(total)
    assert shorter >= 10 and longer >= 10, (shorter, longer)  # at least three strips at S = 7, both ways round
    if name in ST.TIE_SCORINGS:                               # the tie rule is exercised across a seam
        assert sensitive_across_a_seam >= 1


def test_strip_schedule_under_all_flag_combinations():
    total = new_total()
    lost = pairs = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = osc_of(spec)
        alpha = b"ACac" + (b"N" if spec["wildcards"] else b"")
        for a, b, w in pairs_of(2600 + idx, N_FLAG_PAIRS, N_FLAG_LONG, alpha):
            want, _ = models_and_want(osc, a, b, w, total)
            pairs += 1
            if want is None:
                assert flags[2] or flags[3] or flags[4], (flags, a, b, w)      # only a scoring that forbids moves loses a pair
                lost += 1
    print("pairs", pairs, "without an alignment inside the band", lost, total)
    assert_covered(total)
    assert lost >= 50, lost
