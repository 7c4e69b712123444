"""CPU tier: the argument that tests/test_gpu_magnitude.py tests what it claims -- on the oracle and an exact-integer
restatement of the recurrence alone (tests/maglib.py).

For every (family, pair) the GPU file runs: every add the reference's C performs stays inside int32 (the input is defined
upstream: that is the admission to the matrix); the oracle's matrices are the exact ones; the peak crosses the power of two
the family is named for, the top families stand in [2^30, 2^31); the planted gap is on the oracle's alignment; the at-the-floor
families form floor + penalty == INT32_MIN beside cells that are not at the floor; the bands hold or cut the planted path as
the band lists say; and the documented admission rule (include/seqalign_hip.h, SEQALIGN_E_DOMAIN), restated in maglib, refuses
no group whose exact peak leaves room for the widest de-trend.
"""
import importlib.util
from pathlib import Path

import pytest

import bandlib as BL
import bandswlib as BS
import maglib as G
import orclib as O

FAMS = pytest.mark.parametrize("fam", G.FAMILIES, ids=G.family_id)
ARGUED = [f for f in G.FAMILIES if G.argued(f[0], "gapb") or G.argued(f[0], "gapa")]


@FAMS
def test_inputs_are_defined_upstream_and_reach_their_magnitude(fam):
    """Every group of the family: all sums inside int32, oracle == exact integers cell for cell, and the largest |value| of
    the group's pairs in [2^p, 2^(p + 1)) -- for the top families in [2^30, 2^31 - 1 - the largest |penalty|]."""
    for _, shape, is_sw, cs in G.groups(fam):
        peaks = []
        for c in cs:
            e = G.exact(c)
            assert e.fits_int32(), (c.id, e.lo, e.hi)
            rc, M, A, B = O.oracle_fill(c.osc(), c.a, c.b, c.is_sw)
            assert rc == 0 and M.tolist() == e.M and A.tolist() == e.A and B.tolist() == e.B, c.id
            if not is_sw:
                assert e.floor == G.INT32_MIN + abs(c.osc().min_penalty)
            peaks.append(e.peak)
        low = 2 ** (30 if fam[1] == G.TOP else fam[1])
        high = 2 ** 31 - 1 - max(abs(v) for v in G.numbers(cs[0].spec)) if fam[1] == G.TOP else 2 * low - 1
        assert low <= max(peaks) <= high, (G.family_id(fam), shape, is_sw, peaks)
        print(f"{G.family_id(fam)} {shape} {'sw' if is_sw else 'nw'}: scale {cs[0].scale}, peak |value| per pair {peaks}, "
              f"largest value {max(G.exact(c).top for c in cs)}")


def _alignment_gaps(c):
    if c.is_sw:
        rc, hits = O.oracle_sw(c.osc(), c.a, c.b, 1, 1)
        assert rc == 0 and hits, c.id
        h = hits[0]
        return {(w, k + (h["pos_a"] if w == "b" else h["pos_b"])) for w, k in G.gaps_of(h["a"], h["b"])}
    rc, _, ra, rb = O.oracle_nw(c.osc(), c.a, c.b)
    assert rc == 0
    return G.gaps_of(ra, rb)


@pytest.mark.parametrize("fam", ARGUED, ids=G.family_id)
def test_planted_gaps_lie_on_the_oracles_alignment(fam):
    """The planted pairs of every family maglib.argued names: the oracle's global alignment, and its first local hit, pass
    through the planted gap -- a letter of seq_a PLANT columns before the end against '-' (gap_b), or the same in seq_b."""
    n = 0
    for c in G.cases_of(fam=fam):
        want = G.planted(c.shape, c.kind)
        if G.argued(fam[0], c.kind):
            got = _alignment_gaps(c)
            assert set(want) <= got, (c.id, want, sorted(got)[-4:])
            n += len(want)
    assert n >= 5, n
    print(f"{G.family_id(fam)}: {n} planted gaps on the oracle's alignments")


@pytest.mark.parametrize("base", G.FLOOR_BASES)
def test_floor_families_stand_at_the_floor(base):
    """Some penalty equals -|min_penalty|: a sum floor + penalty == INT32_MIN is formed in every pair, and a cell holding
    exactly INT32_MIN + |min_penalty| has a neighbour (left, above or diagonal, any matrix) above the floor."""
    spec1 = G.BASES[base]
    assert -abs(G.min_penalty(spec1)) in G.numbers(spec1)[1:] + [spec1["init"][2] + spec1["init"][3]]
    for c in G.cases_of(fam=(base, 29)):
        e = G.exact(c)
        assert e.lo == G.INT32_MIN, (c.id, e.lo)
        assert abs(G.min_penalty(c.spec)) >= 2 ** 20, c.id          # the floor far above INT32_MIN
        W = len(c.a) + 1
        found = 0
        for X in (e.M, e.A, e.B):
            for idx in range(W + 1, len(X)):
                if X[idx] == e.floor and idx % W and any(Y[k] > e.floor for Y in (e.M, e.A, e.B) for k in (idx - 1, idx - W, idx - W - 1)):
                    found += 1
        assert found, c.id
        print(f"{c.id}: {found} floor cells beside cells above the floor, |min_penalty| {abs(G.min_penalty(c.spec))}")


def test_the_admission_rule_refuses_no_group_with_room():
    """maglib.admitted, the documented rule: every group whose exact peak plus the widest frame's de-trend plus |gap_open| stays
    below 2^31 - 1 is admitted by every class of call -- those that fill whole matrices (frames of up to 4 096 columns), the
    score family and the banded calls (1 024); every family below 2^23 is admitted everywhere; every shape keeps an admitted
    top group for NW and for SW in every class of call; and the rule does refuse something: the flat top groups under SW, whose
    de-trended gap_b sums leave int32."""
    kept, refused = set(), 0
    for fam, shape, is_sw, cs in G.groups():
        la, lb = G.group_lengths(cs)
        for call in G.CALLS:
            adm = G.admitted(cs[0].spec, la, lb, call)
            assert adm or not G.must_be_admitted(cs, call), (G.family_id(fam), shape, is_sw, call)
            assert adm or fam[1] == G.TOP or fam[1] >= 23, (G.family_id(fam), shape, is_sw, call)
            if fam[1] == G.TOP and adm:
                kept.add((shape, is_sw, call))
            refused += not adm
    assert {(s, w, call) for s, _, _ in G.SHAPES for w in (0, 1) for call in G.CALLS} <= kept, kept
    flat = [cs for fam, shape, is_sw, cs in G.groups(("flat", G.TOP), 1)]
    assert flat and not any(G.admitted(cs[0].spec, *G.group_lengths(cs), call) for cs in flat for call in G.CALLS)
    print(f"{refused} (group, call class) combinations refused; top groups kept: {len(kept)}")


@pytest.mark.parametrize("fam", ARGUED, ids=G.family_id)
def test_bands_hold_or_cut_the_planted_path(fam):
    """maglib.sw_bands / nw_bands: under a band marked `holds` the banded result is the unbanded one, under the others it is
    not (bandswlib / bandlib: the banded definitions over the oracle's lookup)."""
    for c in G.cases_of(fam=fam):
        if not G.argued(fam[0], c.kind, bands=True):
            continue
        if c.is_sw:
            rc, full = O.oracle_sw(c.osc(), c.a, c.b, 1, 1)
            for lo, hi, holds in G.sw_bands(c.shape, c.kind):
                _, hit = BS.expected(c.osc(), c.a, c.b, lo, hi)
                assert (([hit] if hit else []) == full) == holds, (c.id, lo, hi)
        else:
            rc, s, ra, rb = O.oracle_nw(c.osc(), c.a, c.b)
            for w, holds in G.nw_bands(c.shape, c.kind):
                assert (BL.expected(c.osc(), c.a, c.b, w) == (s, ra, rb)) == holds, (c.id, w)


def test_fuzzer_scale_redraws_stay_under_one_trial_in_four():
    """seq-align_amd/tools/fuzz_calls.py with scale = 2^23, drawing only (no device): over 200 trials of the seeds the soak
    slice uses, at most one trial in four redraws its factor, and the default scale of 1 draws no factor at all."""
    tools = Path(__file__).resolve().parent.parent / "seq-align_amd" / "tools"
    spec = importlib.util.spec_from_file_location("dry_fuzz_calls", tools / "fuzz_calls.py")
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    for seed in (20261019, 3):
        r = fz.run(seconds=120.0, seed=seed, max_trials=100, scale=1 << 23, dry=True)
        assert r["trials"] == 100 and 4 * r["redrawn_trials"] <= r["trials"], r
        print(f"seed {seed}: {r['redrawn_trials']} of {r['trials']} trials redrew their factor ({r['redraws']} redraws)")
    plain = fz.run(seconds=30.0, seed=20261018, max_trials=5, dry=True)
    assert plain["redraws"] == 0 and plain["trials"] == 5
