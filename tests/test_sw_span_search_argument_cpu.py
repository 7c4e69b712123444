"""CPU tier: the lemma seqalign_sw_span_search's second stage rests on, checked on the oracle without a device.

The search selects its hits from scores and best cells alone (seqalign_sw_score_search) and computes the spans afterwards, for
the selected hits only, on the PREFIX pair of each: (query[0 : end_a], target[0 : end_b]), cut at the full pair's best cell.
That is exact because the first hit of the prefix pair is the full pair's first hit in all five fields, under every flag:
the SW fill is causal; no_end_gap_penalty touches only gap cells of the last row and column, which feed no match cell, so
the prefix's match scores are the full pair's; the first cell in hit order (score descending, column ascending, row
ascending) of the full pair lies in the prefix and is first there too; and the walk leaves the last row and column with its
first step.
"""
import itertools

import pytest

import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

# the scorings of tests/test_sw_span_argument_cpu.py
SCORINGS = {
    "dna_sw": ({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}, b"ACGT"),
    "blosum62": ({"preset": "BLOSUM62"}, b"ARNDCQEGHILKMFPSTWYV"),
    "open0": ({"init": [2, -1, 0, -1, 0, 0, 0, 0, 0, 0]}, b"AC"),
    "ext0": ({"init": [3, -1, -1, 0, 0, 0, 0, 0, 0, 0]}, b"AC"),
    "ext_pos": ({"init": [2, -3, -2, 1, 0, 0, 0, 0, 0, 0]}, b"ACGT"),
}
FLAGS = ("no_start_gap_penalty", "no_end_gap_penalty", "no_gaps_in_a", "no_gaps_in_b", "no_mismatches")
MAX_LEN = 40


def rand_seq(rng, n, alpha):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


def mutate(rng, s, alpha):
    """A relative of s: substitutions, insertions and deletions, about one in six positions."""
    out = bytearray()
    for ch in s:
        r = int(rng.below(18, 1)[0])
        if r == 0:
            continue
        if r == 1:
            out += rand_seq(rng, 1 + int(rng.below(3, 1)[0]), alpha)
        out.append(alpha[int(rng.below(len(alpha), 1)[0])] if r == 2 else ch)
    return bytes(out)


def pairs_of(seed, n, alpha):
    """Random pairs, relatives, and relatives followed by unrelated tails on both sides (the hit ends inside the pair); then the
    four degenerate pairs."""
    rng = W.Rng(seed)
    pairs = []
    for k in range(n):
        la, lb = (int(x) for x in rng.below(MAX_LEN + 1, 2))
        if k % 3 == 0:
            a, b = rand_seq(rng, la, alpha), rand_seq(rng, lb, alpha)
        elif k % 3 == 1:
            a = rand_seq(rng, la, alpha)
            b = mutate(rng, a, alpha)[:MAX_LEN]
        else:
            core = rand_seq(rng, 8 + la // 3, alpha)
            a = (rand_seq(rng, la // 4, alpha) + core + rand_seq(rng, 3 + lb // 4, alpha))[:MAX_LEN]
            b = (rand_seq(rng, lb // 4, alpha) + mutate(rng, core, alpha) + rand_seq(rng, 3 + la // 4, alpha))[:MAX_LEN]
        pairs.append((a, b))
    return pairs + [(b"", b""), (alpha[:1], b""), (b"", alpha[:1]), (alpha[:1], alpha[:1])]


def first_hit(osc, a, b):
    rc, hits = O.oracle_sw(osc, a, b, 1, 1)
    assert rc == 0, (rc, a, b)
    h = hits[0] if hits else None
    return (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) if h else None


@pytest.mark.parametrize("name", list(SCORINGS))
def test_the_prefix_pair_has_the_full_pairs_first_hit(name):
    spec, alpha = SCORINGS[name]
    n_pairs = with_hit = shorter = 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        sc = S.make_scoring({**spec, "flags": dict(zip(FLAGS, flags))})
        osc = O.Scoring.from_buffer_copy(bytes(sc))
        for a, b in pairs_of(8100 + 37 * len(name) + idx, 24, alpha):
            n_pairs += 1
            full = first_hit(osc, a, b)
            if full is None:
                continue
            with_hit += 1
            end_a, end_b = full[1] + full[3], full[2] + full[4]
            assert 1 <= end_a <= len(a) and 1 <= end_b <= len(b)
            assert first_hit(osc, a[:end_a], b[:end_b]) == full, (name, flags, a, b, full)
            shorter += (end_a, end_b) != (len(a), len(b))
    print(f"{name}: {n_pairs} pairs, {with_hit} with a hit, {shorter} with a prefix strictly shorter than the pair")
    assert 3 * shorter >= n_pairs, (name, n_pairs, with_hit, shorter)      # the comparison is not vacuous
