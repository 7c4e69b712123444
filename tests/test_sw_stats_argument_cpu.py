"""CPU tier: what seqalign_sw_stats_batch's kernels rest on, checked against the oracle without a device.

1. The hit span AND the (matches, mismatches) of the oracle's first hit are a function of the three SW matrices alone and can be
   propagated FORWARD beside them: spanlib.propagate with counts beside the span.  Together with a step-by-step walk that
   counts, the definition gives the oracle's seven values.
2. The kernel's shape IN PACKED FORM -- the stop cell as x | y << 16, the counts as matches | mismatches << 16, Python ints
   masked to 32 bits; two merged payloads per column, the one-bit row rule, strips of 5 to 7 columns with their hand-off, the
   best cell's two words through one 64-bit word -- equals the definition state by state.
3. The tie-dense pairs the GPU tests use do tell the walker's priority from its reverse, on the counts alone.
4. The packed words at their limits.
"""
import itertools

import pytest

import orclib as O
import statlib as ST
import swstatlib as SS
from seqalign_amd import workloads as W

INITS = {"dna": [1, -2, -4, -1], "open0": [2, -1, 0, -1], "ext0": [3, -1, -1, 0], "ties": [1, 0, 0, 0], "ext_pos": [2, -3, -2, 1]}


def osc_of(spec):
    return O.build_scoring(spec, "oracle")


def rand_seq(rng, n, alpha):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


def mutate(rng, s, alpha):
    out = bytearray()
    for ch in s:
        r = int(rng.below(18, 1)[0])
        if r == 0:
            continue
        if r == 1:
            out += rand_seq(rng, 1 + int(rng.below(3, 1)[0]), alpha)
        out.append(alpha[int(rng.below(len(alpha), 1)[0])] if r == 2 else ch)
    return bytes(out)


def small_pairs(seed, n, alpha, max_len=28):
    rng = W.Rng(seed)
    pairs = []
    for k in range(n):
        la, lb = (int(x) for x in rng.below(max_len + 1, 2))
        a = rand_seq(rng, la, alpha)
        b = mutate(rng, a, alpha)[:max_len] if k % 2 else rand_seq(rng, lb, alpha)
        pairs.append((a, b))
    return pairs + [(b"", b""), (alpha[:1], b""), (b"", alpha[:1]), (alpha[:1], alpha[:1])]


def check_pair(osc, a, b, want, strips=(1 << 30, 5, 6)):
    """definition == walk == the packed kernel model (state by state) == the oracle's first hit and its counted strings."""
    res, pay = SS.forward(osc, a, b)
    assert res == want, ("forward", a, b, res, want)
    assert SS.walk(osc, a, b) == want, ("walk", a, b)
    for strip in strips:
        assert SS.kernel_model(osc, a, b, strip, pay) == want, ("kernel model", strip, a, b)


@pytest.mark.parametrize("name", list(INITS))
def test_forward_definition_and_packed_model_equal_the_oracles_hit(name):
    alpha = b"AC" if name in ("open0", "ext0", "ties") else b"ACGT"
    osc = osc_of(ST.init_spec(INITS[name]))
    pairs = small_pairs(8300 + len(name), 40, alpha)
    want = SS.want_sw_stats(osc, pairs)
    hits = reversed_differs = 0
    for (a, b), w in zip(pairs, want):
        check_pair(osc, a, b, w)
        rev = SS.forward(osc, a, b, SS.REVERSED)[0]        # another priority: the walk with it, and maybe other counts
        assert rev == SS.walk(osc, a, b, SS.REVERSED), (name, a, b)
        hits += w[0] > 0
        reversed_differs += rev[5:] != w[5:]
    assert hits >= 30
    if name in ("ext0", "ties", "ext_pos"):
        assert reversed_differs >= 1


def test_all_flag_combinations():
    """The 32 flag combinations (test_gpu_score.py's specs) on small pairs with mixed case, a wildcard and directed mutations:
    substitution scores, wildcards and no_mismatches play no part in which bucket a column falls into, case folding does."""
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
@pytest.mark.parametrize("width", ST.TIE_WIDTHS)
def test_tie_dense_pairs_tell_the_priorities_apart(name, width):
    """statlib.tie_pairs with their default seeds: at least TIE_MIN of 40 change their counts under REVERSED, on the oracle
    alone."""
    osc = osc_of(ST.init_spec(ST.TIE_SCORINGS[name]))
    n = SS.tie_sensitive(osc, ST.tie_pairs(name, width))
    print(f"{name} width {width}: {n} of 40 pairs change their counts under the reversed priority")
    assert n >= ST.TIE_MIN, (name, width, n)


def test_packed_words_at_their_limits():
    top = SS.MAX_LEN
    assert top == 65535
    w0 = SS.pack_cell(top, top)
    assert w0 == 0xFFFFFFFF and SS.unpack_cell(w0) == (top, top)
    assert SS.unpack_cell(SS.pack_cell(top, 0)) == (top, 0) and SS.unpack_cell(SS.pack_cell(0, top)) == (0, top)
    w1 = 0
    for _ in range(top):
        w1 = SS.count_step(w1, True)
    assert w1 == 0x0000FFFF and SS.unpack_counts(w1) == (top, 0)          # 65 535 matches plus nothing: no carry
    w1 = 0
    for _ in range(top):
        w1 = SS.count_step(w1, False)
    assert w1 == 0xFFFF0000 and SS.unpack_counts(w1) == (0, top)
    # matches + mismatches <= min(len_a, len_b) <= 65 535: any split of the most columns a walk can have round-trips
    for m in (0, 1, 32767, 32768, 65534, 65535):
        w1 = SS.pack_counts(m, top - m)
        assert SS.unpack_counts(w1) == (m, top - m)
        if m:
            assert SS.count_step(SS.pack_counts(m - 1, top - m), True) == w1
        if m < top:
            assert SS.count_step(SS.pack_counts(m, top - m - 1), False) == w1
    u64 = (SS.pack_cell(top, 1) << 32) | SS.pack_counts(2, 3)             # reduce_best's word
    assert SS.unpack_cell(u64 >> 32) == (top, 1) and SS.unpack_counts(u64 & SS.MASK) == (2, 3)
