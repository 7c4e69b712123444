"""CPU tier: what seqalign_sw_span_banded's kernel rests on, checked against the oracle without a device.

1. The definition of 3.18 holds in a band.  With one rule more -- a cell outside the band is a stop: it holds 0 and its span
   is the cell itself -- the span propagated FORWARD over the banded matrices (bandswlib.fill) is the oracle's first hit over
   them, under the five scorings of test_sw_span_argument_cpu.py and under all 32 flag combinations; the walker always finds
   a predecessor (SEQALIGN_E_TRACEBACK cannot occur).
2. Conditions on the inputs, asserted on the oracle alone: enough hits; with a gap that pays a good share of the hits START
   outside the band, with gap_extend <= 0 none does; the tie-dense scorings tell the walker's priority from the reversed one.
3. The kernel's frame bookkeeping (bandspanlib.frame_model: the shift, the edge cell's V, the feed, the retire, the end pick)
   at a frame of 8 positions against bands of width 1 .. 8 gives the same five fields.
4. The tie-dense GPU batches (spanlib.tie_pairs at widths 200 and 400, bands of +-20 and +-150) each hold a pair whose wanted
   span changes under the reversed priority.
"""
import itertools

import pytest

import bandspanlib as BSP
import spanlib as SP
from test_sw_span_argument_cpu import SCORINGS, oracle_scoring

N_PAIRS, N_FLAG_PAIRS = 300, 40


def wanted(osc, a, b, lo, hi):
    return BSP.want(osc, a, b, lo, hi)[1]


@pytest.mark.parametrize("name", list(SCORINGS))
def test_forward_propagation_over_the_banded_matrices_equals_the_oracles_banded_hit(name):
    spec, alpha = SCORINGS[name]
    osc = oracle_scoring(spec)
    hits = outside = differs_from_unbanded = reversed_differs = 0
    for a, b, lo, hi in BSP.band_pairs(9100 + len(name), N_PAIRS, alpha):
        want = wanted(osc, a, b, lo, hi)
        mats = BSP.banded_mats(osc, a, b, lo, hi)
        assert SP.span_by_propagation(osc, a, b, mats=mats) == want, (name, a, b, lo, hi)      # NoPredecessor would raise
        hits += want[0] > 0
        outside += BSP.starts_outside(want, len(a), len(b), lo, hi)
        differs_from_unbanded += want[0] > 0 and want != wanted(osc, a, b, -len(b), len(a))
        reversed_differs += SP.span_by_propagation(osc, a, b, SP.REVERSED, mats=mats) != want
    print(name, "hits", hits, "start outside the band", outside, "differ from the unbanded hit", differs_from_unbanded,
          "change under M > B > A", reversed_differs)
    assert hits >= 150, hits
    assert differs_from_unbanded * 2 >= hits          # the band matters: most hits are not the unbanded ones
    if osc.gap_extend <= 0:
        assert outside == 0
    if name == "ext_pos":
        assert outside * 4 >= hits, (outside, hits)
    if name in ("open0", "ext0", "ext_pos"):
        assert reversed_differs >= 1


def test_propagation_under_all_flag_combinations():
    """test_kernel_shape_under_all_flag_combinations' scorings, 40 banded pairs each."""
    hits = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = oracle_scoring(spec)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        for a, b, lo, hi in BSP.band_pairs(700 + idx, N_FLAG_PAIRS, alpha):
            want = wanted(osc, a, b, lo, hi)
            assert SP.span_by_propagation(osc, a, b, mats=BSP.banded_mats(osc, a, b, lo, hi)) == want, (flags, a, b, lo, hi)
            hits += want[0] > 0
    assert hits >= 32 * N_FLAG_PAIRS // 3, hits


@pytest.mark.parametrize("name", list(SCORINGS))
def test_frame_bookkeeping_equals_the_oracle(name):
    """Rules 1-3 at a frame of 8 positions: bands of width 1 .. 8, so a full frame (width = F), frames that never move, frames
    that move from row 1 on and bands that start at a late row all occur."""
    spec, alpha = SCORINGS[name]
    osc = oracle_scoring(spec)
    hits = full = moved = 0
    for a, b, lo, hi in BSP.band_pairs(9700 + len(name), N_PAIRS, alpha, max_width=8):
        want = wanted(osc, a, b, lo, hi)
        assert BSP.frame_model(osc, a, b, lo, hi, 8) == want, (name, a, b, lo, hi)
        hits += want[0] > 0
        full += want[0] > 0 and hi - lo + 1 == 8
        moved += want[0] > 0 and want[2] + want[4] + max(lo, -len(b)) >= 2      # the frame had moved by the hit's last row
    assert hits >= 150 and full >= 10 and moved >= 50, (hits, full, moved)


def test_frame_bookkeeping_under_all_flag_combinations():
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = oracle_scoring(spec)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        for a, b, lo, hi in BSP.band_pairs(800 + idx, N_FLAG_PAIRS, alpha, max_width=8):
            assert BSP.frame_model(osc, a, b, lo, hi, 8) == wanted(osc, a, b, lo, hi), (flags, a, b, lo, hi)


def test_tie_dense_gpu_batches_are_tie_sensitive_inside_their_bands():
    """Every batch that tests/test_gpu_sw_span_banded.py runs for ties has at least one pair whose wanted span changes under
    the reversed priority (the counts are recorded in DESIGN.md 3.19).  The batches are spanlib.tie_pairs' 40 pairs; the one
    of them that holds no such pair is run with the generator's next 40 as well (bandspanlib.TIE_N)."""
    assert SP.tie_pairs("ext_pos", 400, n=80)[:40] == SP.tie_pairs("ext_pos", 400)
    counts = BSP.tie_counts(lambda name: oracle_scoring({"init": [*SP.TIE_SCORINGS[name], 0, 0, 0, 0, 0, 0]}))
    print(counts)
    assert len(counts) == 12 and all(n >= 1 for n in counts.values()), counts
