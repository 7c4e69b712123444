"""CPU tier: what the seqalign_sw_gaps_* kernels rest on, checked against the oracle without a device.

1. The numbers of '-' runs in the two strings of the oracle's first hit (swgaplib.want_gaps) are a function of the three SW
   matrices alone and can be carried FORWARD beside them: swgaplib.forward, the definition -- a gap state adds one unless the
   predecessor the walker picks is the same gap state and is not a stop -- equals a step-by-step walk and the counted strings.
2. The sweep's shape with the payload of a state two plain ints and every feed, hand-off and stop RAW (swgaplib.kernel_model:
   the increment decided in the consuming cell, strips of 5 to 7 columns) equals the definition state by state.  Under the five
   scorings of test_sw_counts_argument_cpu.py plus two more with gap_extend > 0, the 32 flag combinations, statlib.tie_pairs and
   denselib's families.
3. The same with bands (swgaplib.frame_model) against the oracle's banded hit, state by state over the banded matrices.
4. The inputs bite, on the oracle alone: runs that begin by extending out of a stop, counts that change under the reversed
   priority, runs in both strings -- and a model that counts open moves gets the first group wrong.
"""
import itertools

import pytest

import bandspanlib as BSP
import bandswlib as BS
import denselib as D
import orclib as O
import statlib as ST
import swgaplib as SG
from seqalign_amd import workloads as W
from test_sw_stats_argument_cpu import INITS, osc_of, small_pairs

# the counts tests' five and two more whose gaps pay: open1 = -1 and open1 = 0
GAP_INITS = dict(INITS, ext_pos2=[3, -2, -3, 2], ext_open0=[2, -3, -1, 1])
EXT_POS = ("ext_pos", "ext_pos2", "ext_open0")
BAND_SCORINGS = {"plain": ([2, -3, -4, -1], b"ACGT"), "ext0": ([3, -1, -1, 0], b"AC"), "ext_pos": ([2, -3, -2, 1], b"ACGT"),
                 "ext_pos2": ([3, -2, -3, 2], b"ACGT")}


def alpha_of(name):
    return b"AC" if name in ("open0", "ext0", "ties") else b"ACGT"


def pairs_of(name):
    return small_pairs(8300 + len(name), 30, alpha_of(name)) + SG.gap_rich_pairs(4100 + len(name), 30, alpha_of(name))


def check_pair(osc, a, b, want, strips=(1 << 30, 5, 6)):
    """definition == walk == the two-int model (state by state) == the '-' runs of the oracle's first hit, its best cell."""
    res, pay = SG.forward(osc, a, b)
    assert res == want, ("forward", a, b, res, want)
    walked, out_of_stop = SG.walk(osc, a, b)
    assert walked == want, ("walk", a, b, walked, want)
    rc, M, _, _ = O.oracle_fill(osc, a, b, 1)
    assert rc == 0
    assert want[:3] == BS.best_cell(M, len(a)), ("best cell", a, b)
    for strip in strips:
        assert SG.kernel_model(osc, a, b, strip, pay) == want, ("kernel model", strip, a, b)
    return out_of_stop


@pytest.mark.parametrize("name", list(GAP_INITS))
def test_two_int_model_equals_the_definition_state_by_state(name):
    osc = osc_of(ST.init_spec(GAP_INITS[name]))
    pairs = pairs_of(name)
    hits = both = 0
    for (a, b), w in zip(pairs, SG.want_gaps(osc, pairs)):
        check_pair(osc, a, b, w)
        hits += w[0] > 0
        both += w[3] > 0 and w[4] > 0
    assert hits >= 50 and both >= 10, (hits, both)


def test_the_inputs_bite():
    """On the oracle alone, over every scoring's pairs: at least 20 pairs hold a run whose first column extends out of a stop,
    at least 20 change a count under the reversed priority, at least half have a run in each string.  And on every pair of the
    first group a model that counts open moves disagrees with the oracle's strings."""
    total = out_of_stop = reversed_differs = both = naive_wrong = 0
    groups = [(name, GAP_INITS[name], SG.gap_rich_pairs(4100 + len(name), 30, alpha_of(name))) for name in GAP_INITS]
    groups += [(name, ST.TIE_SCORINGS[name], ST.tie_pairs(name, ST.TIE_WIDTHS[0])[:20]) for name in ST.TIE_SCORINGS]
    for name, init, pairs in groups:
        osc = osc_of(ST.init_spec(init))
        for (a, b), w in zip(pairs, SG.want_gaps(osc, pairs)):
            total += 1
            both += w[3] > 0 and w[4] > 0
            walked, n = SG.walk(osc, a, b)
            assert walked == w
            reversed_differs += SG.walk(osc, a, b, SG.REVERSED)[0][3:] != w[3:]
            if n:
                out_of_stop += 1
                naive = SG.naive_open_moves(osc, a, b)
                assert naive[:3] == w[:3] and naive[3] + naive[4] == w[3] + w[4] - n, (name, a, b, naive, w, n)
                naive_wrong += naive != w
    assert out_of_stop >= 20 and naive_wrong == out_of_stop, (out_of_stop, naive_wrong)
    assert reversed_differs >= 20, reversed_differs
    assert 2 * both >= total, (both, total)


def test_all_flag_combinations():
    gapped = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        ext = 1 if idx % 5 == 2 else -1                     # some with a gap_extend that pays
        spec = {"init": [1, mismatch, -4 if ext < 0 else -2, ext, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        osc = osc_of(spec)
        batch = W.ragged(8, seed=900 + idx, max_len=30, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        pairs = [(batch.seq_a(p), batch.seq_b(p)) for p in range(batch.n_pairs)] + SG.gap_rich_pairs(300 + idx, 4, b"ACGTacgt", 30)
        for (a, b), w in zip(pairs, SG.want_gaps(osc, pairs)):
            check_pair(osc, a, b, w, strips=(1 << 30, 7))
            gapped += w[3] + w[4] > 0
    assert gapped >= 32, gapped


@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_tie_sensitive_pairs(name):
    """statlib.tie_pairs at the narrowest width: definition == walk == the oracle's strings, and the model equals the definition
    state by state -- strips of 7 and 64 columns, seams included; some pair changes a count under M > B > A."""
    osc = osc_of(ST.init_spec(ST.TIE_SCORINGS[name]))
    pairs = ST.tie_pairs(name, ST.TIE_WIDTHS[0])[:12]
    differs = 0
    for (a, b), w in zip(pairs, SG.want_gaps(osc, pairs)):
        check_pair(osc, a, b, w, strips=(7, 64))
        differs += SG.walk(osc, a, b, SG.REVERSED)[0][3:] != w[3:]
    if name != "ext_pos":        # (there the reversed priority moves the path at this width, not the number of its runs)
        assert differs >= 1, differs


TIE_BANDS = ((-6, 6), (-20, 20), (3, 30))


@pytest.mark.parametrize("name", list(ST.TIE_SCORINGS))
def test_band_frame_on_tie_sensitive_pairs(name):
    """The same pairs inside bands: the oracle's banded hit == the definition over the banded matrices == the frame model, state
    by state."""
    osc = osc_of(ST.init_spec(ST.TIE_SCORINGS[name]))
    hits = gapped = 0
    for a, b in ST.tie_pairs(name, ST.TIE_WIDTHS[0])[:8]:
        for lo, hi in TIE_BANDS:
            w = check_band(osc, a, b, lo, hi, F=64)
            hits += w[0] > 0
            gapped += w[3] + w[4] > 0
    assert hits >= 16 and gapped >= 8, (hits, gapped)


@pytest.mark.parametrize("scoring", D.SW_SCORINGS)
def test_band_frame_on_gap_dense_families(scoring):
    """denselib's alternation and spaced pairs at their smallest inside denselib.sw_bands' bands (the whole matrix, the hit's
    excursion, I->D only, D->I only, the main diagonal alone, a wide band, a band the hit lies outside)."""
    osc = D.oracle_scoring(scoring)
    pairs = [D.alternation(31, 40, k, D.matches_of(scoring)) for k in range(2)] + [D.spaced(31, 40, 7, 1)]
    gapped = 0
    for a, b in pairs:
        for lo, hi in D.sw_bands(31, 40):
            w = check_band(osc, a, b, lo, hi, F=128)
            gapped += w[3] > 0 and w[4] > 0
    assert gapped >= 3, gapped


@pytest.mark.parametrize("scoring", D.SW_SCORINGS)
def test_gap_dense_families(scoring):
    """denselib's shapes at their smallest: an insertion directly against a deletion is two runs, one in each string."""
    osc = D.oracle_scoring(scoring)
    pairs = [D.alternation(31, 40, k, D.matches_of(scoring)) for k in range(3)] + [D.spaced(31, 40, 7 + k, k) for k in range(3)] \
        + [D.staircase(31, 40)]
    adjacent = 0
    for (a, b), w in zip(pairs, SG.want_gaps(osc, pairs)):
        check_pair(osc, a, b, w, strips=(1 << 30, 6))
        rc, hits = O.oracle_sw(osc, a, b, 1, 1)
        adjacent += bool(hits) and D.count_id(hits[0]["a"].encode(), hits[0]["b"].encode()) + D.count_di(hits[0]["a"].encode(), hits[0]["b"].encode()) > 0
    assert adjacent >= 1, adjacent


def check_band(osc, a, b, lo, hi, F=8):
    cell, want = SG.band_want(osc, a, b, lo, hi)
    assert want[:3] == cell, (a, b, lo, hi, want, cell)                   # the banded score call's three
    mats = BSP.banded_mats(osc, a, b, lo, hi)
    res, pay = SG.forward(osc, a, b, mats=mats)
    assert res == want, ("forward", a, b, lo, hi, res, want)
    got = SG.frame_model(osc, a, b, lo, hi, F, pay)
    assert got == want, (a, b, lo, hi, got, want)
    return want


@pytest.mark.parametrize("name", list(BAND_SCORINGS))
def test_band_frame_with_two_ints_equals_the_oracle(name):
    init, alpha = BAND_SCORINGS[name]
    osc = osc_of({"init": [*init, 0, 0, 0, 0, 0, 0]})
    hits = gapped = 0
    for a, b, lo, hi in BSP.band_pairs(9700 + len(name), 300, alpha, max_width=8):
        w = check_band(osc, a, b, lo, hi)
        hits += w[0] > 0
        gapped += w[3] + w[4] > 0
    assert hits >= 150 and gapped >= 5, (hits, gapped)


def test_band_frame_under_all_flag_combinations():
    hits = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = osc_of(spec)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        for a, b, lo, hi in BSP.band_pairs(800 + idx, 40, alpha, max_width=8):
            hits += check_band(osc, a, b, lo, hi)[0] > 0
    assert hits >= 32 * 40 // 3, hits


def test_constructed_pair_holds_on_the_oracle_at_a_small_size():
    """swgaplib.deleted_block at 400 letters: one hit over the whole of both, one run of 40 in string b."""
    a, b = SG.deleted_block(W.Rng(5), 400, 200, 40)
    (w,) = SG.want_gaps(osc_of(ST.init_spec(SG.BLOCK_INIT)), [(a, b)])
    assert w[1:] == (400, 360, 0, 1), w
