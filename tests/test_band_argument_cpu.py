"""CPU tier: the argument behind the banded calls' contract, on the oracle alone (no device).

bandlib.fill without a band is the oracle's fill; when the oracle's own alignment of a pair stays inside a band, the banded
score and strings are the oracle's byte for byte; when it does not, the banded score is not above the full one; and a scoring
that forbids moves may leave no alignment inside a band at all.  Every class is counted and must occur."""
import itertools
import json
import random
from pathlib import Path

import numpy as np
import pytest

import bandlib as BL
import orclib as O


def test_banded_definition_against_the_oracle():
    rng = random.Random(20251)
    combos = list(itertools.product([0, 1], repeat=5))
    n_pairs = 320                                     # ten pairs per flag combination
    n_in = n_out = n_none = 0
    for trial in range(n_pairs):
        flags = combos[trial % 32]
        sc = O.build_scoring({"init": [rng.choice([1, 2, 5]), rng.choice([-1, -2, -4]), rng.choice([0, -2, -4, -10]),
                                       rng.choice([-1, -2]), *flags, 0]})
        la = rng.randrange(0, 48)
        a = bytes(rng.choice(b"ACGTacgt") for _ in range(la))
        b = BL.mutate(rng, a, 0.2) if rng.random() < 0.8 else bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 48)))
        lb = len(b)
        rc, Mo, Ao, Bo = O.oracle_fill(sc, a, b, 0)
        assert rc == 0
        M, A, B = BL.fill(sc, a, b)
        assert np.array_equal(M, Mo) and np.array_equal(A, Ao) and np.array_equal(B, Bo), ("restatement differs", trial, flags)
        rc, score, ra, rb = O.oracle_nw_traceback(sc, a, b, Mo, Ao, Bo)
        assert rc == 0
        w = rng.randrange(0, 12)
        got = BL.expected(sc, a, b, w)
        if got is None:
            n_none += 1
            assert BL.expected_score(sc, a, b, w) < -2 ** 30, (trial, flags)   # the end cell holds floor-derived values
            continue
        if BL.in_band(ra, rb, la, lb, w):
            n_in += 1
            assert got == (score, ra, rb), (trial, flags, w)
        else:
            n_out += 1
            assert got[0] <= score, (trial, flags, w)
        assert got[0] == BL.expected_score(sc, a, b, w)
    assert n_in and n_out and n_none, (n_in, n_out, n_none)
    assert n_in + n_out + n_none == n_pairs


def table_scorings():
    """Scorings that a match / mismatch pair cannot restate: a substitution table, a wildcard, mutations that differ by
    direction, case sensitivity (with a mutation between the two cases of one letter)."""
    presets = json.loads((Path(__file__).resolve().parent / "golden" / "presets.json").read_text())
    return {
        "blosum62": (O.build_scoring(presets["BLOSUM62"]["spec"]), b"ARNDCQEGHILKMFPSTWYV"),
        "wildcard": (O.build_scoring({"init": [2, -3, -4, -1, 0, 0, 0, 0, 0, 0], "wildcards": [["N", -1]]}), b"ACGTNacgtn"),
        "wildcard_no_mismatches": (O.build_scoring({"init": [2, -9, -3, -1, 0, 0, 0, 0, 1, 0], "wildcards": [["N", 0]]}), b"ACGTN"),
        "asymmetric": (O.build_scoring({"init": [1, -2, -4, -1, 0, 1, 0, 0, 0, 0],
                                        "mutations": [["a", "c", -3], ["c", "a", 2], ["g", "t", 0]]}), b"ACGTacgt"),
        "case_sensitive": (O.build_scoring({"init": [3, -2, -5, -2, 1, 0, 0, 0, 0, 1], "mutations": [["a", "A", 1]]}), b"ACGTacgt"),
    }


@pytest.mark.parametrize("name", ["blosum62", "wildcard", "wildcard_no_mismatches", "asymmetric", "case_sensitive"])
def test_restatement_with_a_scoring_table(name):
    """bandlib.fill through the table of orc_scoring_lookup is the oracle's fill, and a band that holds the oracle's own
    alignment gives it back; no pair here lacks a score."""
    sc, alpha = table_scorings()[name]
    rng = random.Random(len(name) + 31)
    n_in = 0
    for trial in range(24):
        a = bytes(rng.choice(alpha) for _ in range(rng.randrange(0, 70)))
        b = BL.mutate(rng, a, 0.2, alpha) if trial % 4 else bytes(rng.choice(alpha) for _ in range(rng.randrange(0, 70)))
        rc, Mo, Ao, Bo = O.oracle_fill(sc, a, b, 0)
        assert rc == 0
        M, A, B, unknown = BL.fill_unknown(sc, a, b)
        assert not unknown
        assert np.array_equal(M, Mo) and np.array_equal(A, Ao) and np.array_equal(B, Bo), ("restatement differs", name, trial)
        assert all(np.array_equal(x, y) for x, y in zip(BL.fill(sc, a, b), (Mo, Ao, Bo)))
        rc, score, ra, rb = O.oracle_nw_traceback(sc, a, b, Mo, Ao, Bo)
        if rc != 0:
            continue                                   # (no_mismatches: the oracle itself finds no path)
        w = BL.smallest_band(ra, rb, len(a), len(b))
        assert BL.expected(sc, a, b, w) == (score, ra, rb), (name, trial, w)
        assert BL.expected_score(sc, a, b, w) == score
        n_in += 1
    assert n_in >= 12, n_in


def test_rowwise_fill_equals_the_cell_by_cell_one():
    """The numpy rows of bandlib.fill against the plain loop of bandlib.fill_cells, band edges included: the 32 flag
    combinations, gap_extend of either sign and zero, bands that cut the path, bands wider than the matrix, empty sides."""
    rng = random.Random(99)
    scs = table_scorings()
    n = 0
    for trial, flags in enumerate(list(itertools.product([0, 1], repeat=5)) * 3):
        if trial % 8 == 7:
            sc, alpha = scs[sorted(scs)[(trial // 8) % len(scs)]]
        else:
            sc = O.build_scoring({"init": [rng.choice([1, 2, 5]), rng.choice([-1, -2, -4]), rng.choice([2, 0, -2, -10]),
                                           rng.choice([1, 0, -1, -3]), *flags, trial & 1]})
            alpha = b"ACGTacgt"
        a = bytes(rng.choice(alpha) for _ in range(rng.randrange(0, 40)))
        b = BL.mutate(rng, a, 0.25, alpha) if trial % 3 else bytes(rng.choice(alpha) for _ in range(rng.randrange(0, 40)))
        for band in (None, BL.band_of(len(a), len(b), rng.randrange(0, 6)), BL.band_of(len(a), len(b), 100),
                     (-rng.randrange(0, 4), rng.randrange(0, 9))):
            got, want = BL.fill_unknown(sc, a, b, band), BL.fill_cells(sc, a, b, band)
            assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3], (trial, flags, band, a, b)
            n += 1
    assert n == 384


def test_border_feed_switch_is_the_defect_it_names():
    """bandlib's border_feed (not the definition: what test_gpu_band_edges.py's feed pairs are measured against) changes
    nothing while the band holds the whole border column, never lowers a cell, and lets a straight gap down the border column
    into the band where the definition has the floor."""
    sc = O.build_scoring({"init": [5, -4, -4, -1, 0, 0, 0, 0, 0, 0]})
    a, b = b"WWWWWWWWACGTACGTAC", b"RRRRRRRRRRRRACGTACGTAC"
    whole = BL.band_of(len(a), len(b), len(b))
    assert all(np.array_equal(x, y) for x, y in zip(BL.fill_unknown(sc, a, b, whole, True)[:3], BL.fill(sc, a, b, whole)))
    band = BL.band_of(len(a), len(b), 0)                       # (-4, 0): the core is on diagonal -4
    got, want = BL.fill_unknown(sc, a, b, band, True)[:3], BL.fill(sc, a, b, band)
    assert all((x >= y).all() for x, y in zip(got, want))
    W = len(a) + 1
    assert want[2][12 * W + 8] == BL.INT_MIN + 5 and got[2][12 * W + 8] == -4 - 12 - 5   # B of (8, 12): the floor / border + a gap
    assert BL.expected_score(sc, a, b, 0, border_feed=True) > BL.expected_score(sc, a, b, 0)


def test_pair_without_a_score_leaves_the_floor():
    """use_match_mismatch = 0 and one letter pair outside the mutations: the oracle's fill stops there; the restatement
    reports the cells, leaves the floor in their M, and agrees with the oracle on every row above the first of them."""
    sc = O.build_scoring({"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0], "use_match_mismatch": 0,
                          "mutations": [[x, y, 2 if x == y else -1] for x in "acgt" for y in "acgt"] +
                                       [["x", c, -1] for c in "acgt"] + [[c, "y", -1] for c in "acgt"]})
    a, b = b"ACGTXACGTA", b"ACGTTYCGTA"
    assert O.oracle_fill(sc, a, b, 0)[0] != 0
    M, A, B, unknown = BL.fill_unknown(sc, a, b)
    assert unknown == [(5, 6)] == BL.fill_cells(sc, a, b)[3]
    floor = BL.INT_MIN + abs(sc.min_penalty)
    assert M[6 * 11 + 5] == floor
    rc, Mo, Ao, Bo = O.oracle_fill(sc, a, b[:5], 0)
    assert rc == 0 and np.array_equal(M[:5 * 11], Mo[:5 * 11]) and np.array_equal(A[:5 * 11], Ao[:5 * 11])
    assert BL.fill_unknown(sc, a, b, (0, 3))[3] == [] and BL.fill_unknown(sc, a, b, (-1, 0))[3] == [(5, 6)]   # diagonal -1


def test_band_geometry():
    for la, lb, w in [(0, 0, 0), (0, 7, 0), (7, 0, 3), (10, 10, 0), (10, 14, 2), (14, 10, 2), (5, 5, 2 ** 31), (300, 2000000, 0)]:
        d_lo, d_hi = BL.band_of(la, lb, w)
        assert d_lo <= 0 <= d_hi and d_lo <= la - lb <= d_hi            # both corner cells are in every band
        assert -lb <= d_lo and d_hi <= la
        assert BL.width_of(la, lb, w) <= la + lb + 1
    assert BL.width_of(5, 5, 2 ** 31) == 11                               # a band that covers the whole matrix
    assert BL.width_of(300, 2000000, 0) > 1024
    assert BL.width_of(10, 10, 0) == 1
    for la, lb, width in [(100, 100, 63), (100, 103, 64), (3000, 2901, 1024), (3000, 2900, 1023), (40, 0, 41)]:
        w = BL.w_for_width(la, lb, width)
        assert w is not None and BL.width_of(la, lb, w) == width
