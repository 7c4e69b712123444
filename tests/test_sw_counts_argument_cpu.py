"""CPU tier: what the seqalign_sw_counts_* kernels rest on, checked against the oracle without a device.

1. The sweep's shape with the payload of a state LITERALLY two unmasked words (matches, mismatches) and no stop cell
   (swcountlib.kernel_model: two merged payloads per column, the one-bit row rule, strips of 5 to 7 columns with their
   hand-off, the best cell's two words through one 64-bit word) equals, state by state, the cnt half of the definition
   (swstatlib.forward) and of the walk (swstatlib.walk); its result equals swstatlib.want_sw_stats' counts and
   bandswlib.best_cell.  Under the five scorings and the 32 flag combinations of test_sw_stats_argument_cpu.py, on its pair
   generator, and on tie-dense pairs that tell the walker's priority from its reverse.
2. The same with bands: the band frame's bookkeeping over the same two words (swcountlib.frame_model) against
   bandstatlib.want -- the banded score call's cell and the banded statistics call's counts -- and state by state against the
   definition over the banded matrices.
3. A stop is (0, 0) wherever it is: dropping the stop cell changes no count.
"""
import itertools

import pytest

import bandspanlib as BSP
import bandstatlib as BST
import bandswlib as BS
import orclib as O
import statlib as ST
import swcountlib as SC
import swstatlib as SS
from seqalign_amd import workloads as W
from test_sw_stats_argument_cpu import INITS, osc_of, small_pairs

BAND_SCORINGS = {"plain": ([2, -3, -4, -1], b"ACGT"), "ext0": ([3, -1, -1, 0], b"AC"), "ext_pos": ([2, -3, -2, 1], b"ACGT")}


def check_pair(osc, a, b, want7, strips=(1 << 30, 5, 6)):
    """definition == walk == the two-word model (state by state) == the oracle's first hit, its counted strings, its best cell."""
    res, pay = SS.forward(osc, a, b)
    assert res == want7, ("forward", a, b, res, want7)
    want = SC.counts_of(want7)
    assert SC.counts_of(SS.walk(osc, a, b)) == want, ("walk", a, b)
    rc, M, _, _ = O.oracle_fill(osc, a, b, 1)
    assert rc == 0
    assert want[:3] == BS.best_cell(M, len(a)), ("best cell", a, b)
    for strip in strips:
        assert SC.kernel_model(osc, a, b, strip, pay) == want, ("kernel model", strip, a, b)


@pytest.mark.parametrize("name", list(INITS))
def test_two_word_model_equals_the_definition_state_by_state(name):
    alpha = b"AC" if name in ("open0", "ext0", "ties") else b"ACGT"
    osc = osc_of(ST.init_spec(INITS[name]))
    pairs = small_pairs(8300 + len(name), 40, alpha)
    hits = mism = 0
    for (a, b), w in zip(pairs, SS.want_sw_stats(osc, pairs)):
        check_pair(osc, a, b, w)
        hits += w[0] > 0
        mism += w[6] > 0
    assert hits >= 30, hits
    # (under "ties" and "ext_pos" a gap costs no more than a mismatch and the walker takes the gap: no mismatch column; the flag
    # combinations below and the banded pairs are where the second word counts under those)
    if name not in ("ties", "ext_pos"):
        assert mism >= 1, mism


def test_all_flag_combinations():
    mismatches = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        osc = osc_of(spec)
        batch = W.ragged(8, seed=900 + idx, max_len=30, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        pairs = [(batch.seq_a(p), batch.seq_b(p)) for p in range(batch.n_pairs)]
        for (a, b), w in zip(pairs, SS.want_sw_stats(osc, pairs)):
            check_pair(osc, a, b, w, strips=(1 << 30, 7))
            mismatches += w[6]
    assert mismatches > 0


@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_tie_sensitive_pairs(name):
    """statlib.tie_pairs at the narrowest width: pairs whose counts change under M > B > A exist (swstatlib.tie_sensitive, on
    the oracle alone), and on every pair the model keeps the walker's counts -- strips of 7 and 64 columns, seams included."""
    osc = osc_of(ST.init_spec(ST.TIE_SCORINGS[name]))
    pairs = ST.tie_pairs(name, ST.TIE_WIDTHS[0])[:12]
    assert SS.tie_sensitive(osc, pairs) >= 1
    for (a, b), w in zip(pairs, SS.want_sw_stats(osc, pairs)):
        want = SC.counts_of(w)
        assert SC.counts_of(SS.walk(osc, a, b)) == want
        for strip in (7, 64):
            assert SC.kernel_model(osc, a, b, strip) == want, (name, strip, a, b)


def check_band(osc, a, b, lo, hi):
    cell, seven = BST.want(osc, a, b, lo, hi)
    want = SC.counts_of(seven)
    assert want[:3] == tuple(cell), (a, b, lo, hi, want, cell)            # the banded score call's three
    mats = BSP.banded_mats(osc, a, b, lo, hi)
    pay = SS.forward(osc, a, b, mats=mats)[1]
    got = SC.frame_model(osc, a, b, lo, hi, 8, pay)
    assert got == want, (a, b, lo, hi, got, want)
    return seven


@pytest.mark.parametrize("name", list(BAND_SCORINGS))
def test_band_frame_with_two_words_equals_the_oracle(name):
    init, alpha = BAND_SCORINGS[name]
    osc = osc_of({"init": [*init, 0, 0, 0, 0, 0, 0]})
    hits = mism = gapped = 0
    for a, b, lo, hi in BSP.band_pairs(9700 + len(name), 300, alpha, max_width=8):
        w = check_band(osc, a, b, lo, hi)
        hits += w[0] > 0
        mism += w[6] > 0
        gapped += w[0] > 0 and w[3] + w[4] != 2 * (w[5] + w[6])
    assert hits >= 150 and mism >= 1 and gapped >= 1, (hits, mism, gapped)


def test_band_frame_under_all_flag_combinations():
    hits = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = osc_of(spec)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        for a, b, lo, hi in BSP.band_pairs(800 + idx, 40, alpha, max_width=8):
            hits += check_band(osc, a, b, lo, hi)[0] > 0
    assert hits >= 32 * 40 // 3, hits


def test_constructed_pairs_hold_on_the_oracle_at_a_small_size():
    """swcountlib.self_pair / apart_pair at 300 letters: what the GPU tier asserts by construction at 66 000."""
    n = 300
    a, _ = SC.self_pair(W.Rng(5), n)
    assert SC.want_counts(osc_of(ST.init_spec(SC.SELF_INIT)), [(a, a)]) == [(n, n, n, n, 0)]
    assert SC.want_counts(osc_of(ST.init_spec(SC.APART_INIT)), [SC.apart_pair(n)]) == [(n, n, n, 0, n)]
