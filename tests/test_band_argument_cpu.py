"""CPU tier: the argument behind the banded calls' contract, on the oracle alone (no device).

bandlib.fill without a band is the oracle's fill; when the oracle's own alignment of a pair stays inside a band, the banded
score and strings are the oracle's byte for byte; when it does not, the banded score is not above the full one; and a scoring
that forbids moves may leave no alignment inside a band at all.  Every class is counted and must occur."""
import itertools
import random

import numpy as np

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
