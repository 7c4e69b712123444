"""CPU tier: the argument behind the banded SW calls' contract, on the oracle alone (no device).

1. A band that covers every inner cell gives orc_fill(is_sw = 1)'s matrices exactly.
2. Banded values are <= the full ones everywhere; when the full matrix's best-hit walk visits in-band cells only, start and
   end cell included, the banded hit is the full one field for field and byte for byte.
3. Otherwise the banded score is not above the full one.
4. With gap_open + gap_extend <= 0 and gap_extend <= 0 the banded hit's own walk never leaves the band.
Reads of 20-70 letters with 15 % edits planted at a random offset in a window, band = the read's diagonal +- w, w in 0..11,
four scorings, the 32 flag combinations in turn.  Both classes of (2) / (3) are counted and must hold 40 pairs each."""
import itertools
import random

import numpy as np
import pytest

import bandlib as BL
import bandswlib as BS
import orclib as O

SCORINGS = [(1, -1, -2, -1), (2, -3, -4, -1), (5, -4, -10, -2), (3, -2, 0, -2)]   # match, mismatch, gap_open, gap_extend


def _in_band(hit, band):
    lo, hi = BS.hit_excursion(hit)
    return band[0] <= lo and hi <= band[1]


def test_banded_sw_definition_against_the_oracle():
    rng = random.Random(20262)
    combos = list(itertools.product([0, 1], repeat=5))
    n_pairs = 416                                     # thirteen pairs per flag combination
    n_in = n_out = n_lower = n_no_hit = 0
    for trial in range(n_pairs):
        flags = combos[trial % 32]
        sc = O.build_scoring({"init": [*SCORINGS[(trial // 32) % 4], *flags, 0]})
        a, b, offset = BS.read_in_window(rng, rng.randrange(20, 71), rng.randrange(70, 111), 0.15)
        la, lb = len(a), len(b)
        w = rng.randrange(0, 12)
        band = (-offset - w, -offset + w)

        rc, Mo, Ao, Bo = O.oracle_fill(sc, a, b, 1)
        assert rc == 0
        # (1) the whole matrix, and a band that just covers the inner cells
        for whole in (None, (1 - lb, la - 1)):
            M, A, B = BS.fill(sc, a, b, whole)
            assert np.array_equal(M, Mo) and np.array_equal(A, Ao) and np.array_equal(B, Bo), ("restatement differs", trial, flags)

        M, A, B, unknown = BS.fill_unknown(sc, a, b, band)
        assert not unknown
        Mc, Ac, Bc, _ = BS.fill_cells(sc, a, b, band)
        assert np.array_equal(M, Mc) and np.array_equal(A, Ac) and np.array_equal(B, Bc), ("the two fills differ", trial, flags)
        # (2) banded <= full everywhere
        assert (M <= Mo).all() and (A <= Ao).all() and (B <= Bo).all(), (trial, flags)

        rc, full = BS.hit_of(sc, a, b, Mo, Ao, Bo, 1)
        assert rc == 0
        rc, got = BS.hit_of(sc, a, b, M, A, B, 1)
        assert rc == 0
        score = BS.best_cell(M, la)
        assert (got is None) == (score[0] == 0)
        if got is not None:
            assert got["score"] == score[0] and got["pos_a"] + got["len_a"] == score[1] and got["pos_b"] + got["len_b"] == score[2]
            # (4)
            if sc.gap_open + sc.gap_extend <= 0 and sc.gap_extend <= 0:
                assert _in_band(got, band), (trial, flags, band, got)
        if full is None:
            n_no_hit += 1
            assert got is None
            continue
        if _in_band(full, band):
            n_in += 1
            assert got == full, (trial, flags, band)
        else:
            n_out += 1
            assert (got["score"] if got else 0) <= full["score"], (trial, flags, band)
            n_lower += (got["score"] if got else 0) < full["score"]
    assert n_in >= 40 and n_out >= 40, (n_in, n_out)
    assert n_lower, "no band ever cost a pair anything"
    assert n_in + n_out + n_no_hit == n_pairs


@pytest.mark.parametrize("ge", [1, 2])
def test_a_walk_may_leave_the_band_when_gaps_pay(ge):
    """gap_extend > 0 is legal upstream; the banded hit's walk may then step onto a cell outside the band, which reads 0 and
    ends it.  The definition stands: the two fills agree and the hit is the oracle's over the banded matrices."""
    rng = random.Random(77 + ge)
    left = 0
    for trial in range(40):
        sc = O.build_scoring({"init": [2, -3, -ge - rng.randrange(0, 3), ge, 0, 0, 0, 0, 0, 0]})
        a, b, offset = BS.read_in_window(rng, rng.randrange(20, 50), rng.randrange(50, 80), 0.15)
        w = rng.randrange(0, 6)
        band = (-offset - w, -offset + w)
        M, A, B, _ = BS.fill_unknown(sc, a, b, band)
        Mc, Ac, Bc, _ = BS.fill_cells(sc, a, b, band)
        assert np.array_equal(M, Mc) and np.array_equal(A, Ac) and np.array_equal(B, Bc)
        rc, got = BS.hit_of(sc, a, b, M, A, B, 1)
        assert rc == 0 and got is not None
        left += not _in_band(got, band)
    assert left, "no walk left its band"


def test_bounds_anywhere_and_empty_bands():
    sc = O.build_scoring({"init": [2, -3, -4, -1, 0, 0, 0, 0, 0, 0]})
    a, b = b"ACGTACGTAC", b"TTACGTACGG"
    la, lb = len(a), len(b)
    rc, Mo, Ao, Bo = O.oracle_fill(sc, a, b, 1)
    assert rc == 0
    for band in ((-2 ** 31, 2 ** 31 - 1), (-lb, la), (-1000, 1000)):
        assert BS.width_of(la, lb, *band) == la + lb + 1
        assert np.array_equal(BS.fill(sc, a, b, band)[0], Mo)
    for band in ((la + 1, la + 7), (-lb - 9, -lb - 1), (la + 1, 2 ** 31 - 1)):
        assert BS.clip(la, lb, *band) is None and BS.width_of(la, lb, *band) == 0
        assert BS.expected(sc, a, b, *band) == ((0, 0, 0), None)
        assert not BS.fill_cells(sc, a, b, band)[0].any()
    # wholly right of the main diagonal, wholly left of it
    for band in ((3, 5), (-6, -2)):
        M = BS.fill(sc, a, b, band)[0].reshape(lb + 1, la + 1)
        i, j = np.meshgrid(np.arange(la + 1), np.arange(lb + 1))
        outside = (i - j < band[0]) | (i - j > band[1])
        assert not M[outside].any() and M[~outside].any()
        assert np.array_equal(M.ravel(), BS.fill_cells(sc, a, b, band)[0])
