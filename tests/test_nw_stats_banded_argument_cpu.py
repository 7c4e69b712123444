"""CPU tier: what seqalign_nw_stats_banded's kernel rests on, checked against the oracle without a device.

1. The kernel's frame bookkeeping over payloads (bandnwstatlib.frame_model: positions, the three phases of the feed, the shift,
   the reset of V and D of the cell above the right edge, the end pick) at a frame of 8 positions against bands of width 1 .. 8
   gives the banded end value and the counted columns of the oracle's walk over the banded matrices (bandnwstatlib.want), under
   all 32 flag combinations, the three tie scorings and a gap that pays; no band cell reads a position that holds no band cell
   (the model carries POISON there and asserts); every phase of the feed is hit, with len_a < len_b and len_a > len_b.
2. The mark is the rule (bandnwstatlib.want: the oracle's walk, less the documented family).  On these scorings of small numbers
   it agrees with the value: the model's end state carries the mark exactly where the end value is below INT32_MIN / 2, which is
   what the call went by before (tests/test_magnitude_argument_cpu.py has the scorings of large numbers, where the two part).
3. The documented family: pairs on which the oracle's walk "succeeds" although the end value is at the floor (no_mismatches:
   the walker reads a blocked letter pair as score 0).  The call returns SEQALIGN_E_TRACEBACK for them; they occur here.
4. Conditions on the GPU tier's inputs, on the oracle alone: every tie batch and band holds a pair whose counts change under the
   reversed priority; a flag batch loses pairs to SEQALIGN_E_TRACEBACK only under no_mismatches or no_gaps_in_*, and then at
   most a quarter.
"""
import itertools

import pytest

import bandlib as BL
import bandnwstatlib as BN
import bandspanlib as BSP
import orclib as O
import statlib as ST

N_PAIRS, N_FLAG_PAIRS = 200, 60
SCORINGS = {**{name: (init, b"AC") for name, init in ST.TIE_SCORINGS.items()}, "extend_pays": ([3, -4, -9, 1], b"ACGT")}


def osc_of(spec):
    return O.build_scoring(spec, "oracle")


def model_and_want(osc, a, b, w):
    """(the model's three values or None by ITS mark, the wanted three or None by the oracle's WALK); the mark must agree
    with the walk, and here, at small numbers, with the value."""
    got, mark, phases = BN.frame_model(osc, a, b, w, 8)
    want = BN.want(osc, a, b, w)
    assert mark == (got[0] < BN.HALF) == (want is None), (a, b, w, got, mark, want)
    return (None if mark else got), want, phases


@pytest.mark.parametrize("name", list(SCORINGS))
def test_frame_bookkeeping_equals_the_oracle(name):
    init, alpha = SCORINGS[name]
    osc = osc_of(ST.init_spec(init))
    seen = {}                                               # (phase, len_a < len_b) -> pairs
    widths, with_mismatches, with_gaps = set(), 0, 0
    for a, b, w in BN.small_pairs(900 + len(name), N_PAIRS, alpha):
        got, want, phases = model_and_want(osc, a, b, w)
        assert want is not None and got == want, (name, a, b, w, got, want)      # a plain scoring loses no pair
        widths.add(BL.width_of(len(a), len(b), w))
        with_mismatches += want[2] > 0
        with_gaps += 2 * (want[1] + want[2]) != len(a) + len(b)
        if len(a) != len(b):
            for ph in phases:
                seen[ph, len(a) < len(b)] = seen.get((ph, len(a) < len(b)), 0) + 1
    print(name, seen, sorted(widths), with_mismatches, with_gaps)
    assert widths == set(range(1, 9))
    assert set(seen) == {(ph, shorter) for ph in (BN.BORDER, BN.STOPPED, BN.MOVING) for shorter in (False, True)}, seen
    assert min(seen.values()) >= 20, seen
    # both counters move and alignments with gaps occur under every scoring (under "ties" a gap costs nothing, so a mismatch
    # column is rare there)
    assert with_mismatches >= 1 and with_gaps >= 20


def test_frame_bookkeeping_under_all_flag_combinations_and_the_documented_family():
    lost = at_the_floor = total = 0
    phases_seen = set()
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = osc_of(spec)
        alpha = b"ACac" + (b"N" if spec["wildcards"] else b"")
        for a, b, w in BN.small_pairs(600 + idx, N_FLAG_PAIRS, alpha):
            got, want, phases = model_and_want(osc, a, b, w)
            assert got == want, (flags, a, b, w, got, want)
            phases_seen |= phases
            total += 1
            if want is None:
                assert flags[2] or flags[3] or flags[4], (flags, a, b, w)      # only a scoring that forbids moves loses a pair
                lost += 1
                walked = BL.expected(osc, a, b, w)
                if walked is not None:                      # the align call's walker "succeeds": the documented difference
                    assert flags[4] and walked[0] < BN.HALF, (flags, a, b, w, walked)
                    at_the_floor += 1
    print("pairs", total, "without an alignment inside the band", lost, "of which the oracle's walk succeeds at the floor", at_the_floor)
    assert phases_seen == {BN.BORDER, BN.STOPPED, BN.MOVING}
    assert lost >= 100 and at_the_floor >= 5, (lost, at_the_floor)


def test_tie_dense_gpu_batches_change_their_counts_under_the_reversed_priority():
    """Every batch and band that tests/test_gpu_nw_stats_banded.py runs for ties has at least one pair whose (matches,
    mismatches) change under M > B > A over the banded matrices.  A batch is a prefix of statlib.tie_pairs' generator."""
    for (name, width), n in BN.TIE_N.items():
        assert n >= 40 and ST.tie_pairs(name, width, n=n)[:40] == ST.tie_pairs(name, width)
    for name, width in itertools.product(ST.TIE_SCORINGS, BN.TIE_WIDTHS):
        assert all(BL.width_of(len(a), len(b), max(BN.TIE_BANDS)) <= 512 for a, b in BN.tie_batch(name, width))
    counts = BN.tie_counts(lambda name: osc_of(ST.init_spec(ST.TIE_SCORINGS[name])))
    print(counts)
    assert len(counts) == 18 and all(n >= 1 for n in counts.values()), counts


def test_gpu_flag_batches_lose_pairs_only_where_the_scoring_forbids_moves():
    """tests/test_gpu_nw_stats_banded.py's flag batches (bandnwstatlib.flag_pairs): no pair is lost to SEQALIGN_E_TRACEBACK
    unless the scoring has no_mismatches or no_gaps_in_*, and then at most a quarter of the batch; some batch does lose one, so
    the error path runs."""
    losing = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = osc_of(spec)
        pairs = BN.flag_pairs(idx, flags, b"ACGTacgt" + (b"N" if spec["wildcards"] else b""))
        lost = sum(BN.want(osc, a, b, w) is None for a, b, w in pairs)
        assert len(pairs) == BN.FLAG_N and lost <= BN.FLAG_N // 4, (flags, lost)
        if not (flags[2] or flags[3] or flags[4]):
            assert lost == 0, (flags, lost)
        losing += lost > 0
    assert losing >= 8, losing
