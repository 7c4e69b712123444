"""CPU tier: what seqalign_sw_stats_banded's kernel rests on, checked against the oracle without a device.

1. The kernel's frame bookkeeping with counts IN PACKED FORM (bandstatlib.frame_model: the shift, the edge cell's feed, the
   feed left of the frame, the retire and the end pick over payloads (cell word, counts word) masked to 32 bits) at a frame of
   8 positions against bands of width 1 .. 8 gives the seven values of the oracle's banded hit and its counted strings
   (bandstatlib.want), under the plain scoring, ext0 and ext_pos and under all 32 flag combinations; its first five values are
   bandspanlib.want's; and no band cell reads a position that holds no band cell (the model carries POISON there and asserts).
2. Conditions on the inputs, asserted on the oracle alone: enough hits; mismatches occur and hits with gaps occur under every
   scoring; with a gap that pays a share of the hits start outside the band.
3. The tie-dense GPU batches (bandstatlib.tie_batch at widths 200 and 400, bands of +-20 and +-150) each hold a pair whose
   COUNTS change under the reversed priority M > B > A inside the band.
"""
import itertools

import pytest

import bandspanlib as BSP
import bandstatlib as BST
import spanlib as SP
from test_sw_span_argument_cpu import oracle_scoring

N_PAIRS, N_FLAG_PAIRS = 300, 40
# test_gpu_sw_span_banded.WIDTH_SCORINGS as specs
SCORINGS = {"plain": ([2, -3, -4, -1], b"ACGT"), "ext0": ([3, -1, -1, 0], b"AC"), "ext_pos": ([2, -3, -2, 1], b"ACGT")}


def both(osc, a, b, lo, hi):
    """(the frame model's seven, the wanted seven) with the model's first five held against the span call's wanted five."""
    want = BST.want(osc, a, b, lo, hi)[1]
    got = BST.frame_model(osc, a, b, lo, hi, 8)
    assert got[:5] == BSP.want(osc, a, b, lo, hi)[1], (a, b, lo, hi, got)
    return got, want


@pytest.mark.parametrize("name", list(SCORINGS))
def test_frame_bookkeeping_with_packed_counts_equals_the_oracle(name):
    """Bands of width 1 .. 8 at a frame of 8: a full frame (width = F), frames that never move, frames that move from row 1 on
    and bands that start at a late row all occur."""
    init, alpha = SCORINGS[name]
    osc = oracle_scoring({"init": [*init, 0, 0, 0, 0, 0, 0]})
    hits = full = moved = mismatched = gapped = outside = 0
    for a, b, lo, hi in BSP.band_pairs(9700 + len(name), N_PAIRS, alpha, max_width=8):
        got, want = both(osc, a, b, lo, hi)
        assert got == want, (name, a, b, lo, hi, got, want)
        hits += want[0] > 0
        full += want[0] > 0 and hi - lo + 1 == 8
        moved += want[0] > 0 and want[2] + want[4] + max(lo, -len(b)) >= 2      # the frame had moved by the hit's last row
        mismatched += want[6] > 0
        gapped += want[0] > 0 and want[3] + want[4] != 2 * (want[5] + want[6])
        outside += BSP.starts_outside(want[:5], len(a), len(b), lo, hi)
    print(name, "hits", hits, "full frames", full, "moved", moved, "with mismatches", mismatched, "with gaps", gapped,
          "start outside the band", outside)
    assert hits >= 150 and full >= 10 and moved >= 50, (hits, full, moved)
    # both halves of the counts word and a hit with gaps occur under every scoring.  No more is asked: on pairs of at most 32
    # letters a hit rarely affords a mismatch at -3 or a gap at -5; the GPU tier's planted pairs (8 % edits over 130 .. 200
    # rows) are where the counts are large
    assert mismatched >= 1 and gapped >= 1, (mismatched, gapped)
    if osc.gap_extend <= 0:
        assert outside == 0
    else:
        assert outside >= 10, outside


def test_frame_bookkeeping_with_packed_counts_under_all_flag_combinations():
    hits = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = oracle_scoring(spec)
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        for a, b, lo, hi in BSP.band_pairs(800 + idx, N_FLAG_PAIRS, alpha, max_width=8):
            got, want = both(osc, a, b, lo, hi)
            assert got == want, (flags, a, b, lo, hi, got, want)
            hits += want[0] > 0
    assert hits >= 32 * N_FLAG_PAIRS // 3, hits


def test_tie_dense_gpu_batches_change_their_counts_under_the_reversed_priority():
    """Every batch that tests/test_gpu_sw_stats_banded.py runs for ties has at least one pair whose (matches, mismatches)
    change under M > B > A inside the band -- a change of the span alone does not count.  A batch of bandspanlib's that held no
    such pair would be lengthened from the same generator (bandstatlib.TIE_N), never dropped; the batches are prefixes of one
    another."""
    for (name, width), n in BST.TIE_N.items():
        assert SP.tie_pairs(name, width, n=n)[:40] == SP.tie_pairs(name, width)
        assert n >= BSP.TIE_N.get((name, width), 40)
    counts = BST.tie_counts(lambda name: oracle_scoring({"init": [*SP.TIE_SCORINGS[name], 0, 0, 0, 0, 0, 0]}))
    print(counts)
    assert len(counts) == 12 and all(n >= 1 for n in counts.values()), counts
