"""CPU tier: the argument that tests/test_gpu_magnitude.py tests what it claims -- on the oracle and an exact-integer
restatement of the recurrence alone (tests/maglib.py).

For every (family, pair) the GPU file runs: every add the reference's C performs stays inside int32 (the input is defined
upstream: that is the admission to the matrix); the oracle's matrices are the exact ones; the peak crosses the power of two
the family is named for, the top families stand in [2^30, 2^31); the planted gap is on the oracle's alignment; the at-the-floor
families form floor + penalty == INT32_MIN beside cells that are not at the floor; the bands hold or cut the planted path as
the band lists say; and the documented admission rule (include/seqalign_hip.h, SEQALIGN_E_DOMAIN), restated in maglib, refuses
no group whose exact peak leaves room for the widest de-trend.  The deep families hold real global scores and banded end values
in (-2^31, -2^30) that the oracle walks; and each statistics, span and set call of the GPU file's sections G and H meets a group
on either side of the admission rule.
"""
import importlib.util
from pathlib import Path

import pytest

import bandlib as BL
import bandnwstatlib as BN
import bandswlib as BS
import maglib as G
import orclib as O

FAMS = pytest.mark.parametrize("fam", G.FAMILIES, ids=G.family_id)
ARGUED = [f for f in G.FAMILIES if G.argued(f[0], "gapb") or G.argued(f[0], "gapa")]


@FAMS
def test_inputs_are_defined_upstream_and_reach_their_magnitude(fam):
    """Every group of the family: all sums inside int32, oracle == exact integers cell for cell, and the largest |value| of
    the group's pairs in [2^p, 2^(p + 1)) -- for the top families in [2^30, 2^31 - 1 - the largest |penalty|], for the deep ones
    in [2^30, 2^31)."""
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
        low = 2 ** (30 if fam[1] in (G.TOP, G.DEEP) else fam[1])
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
            assert adm or fam[1] in (G.TOP, G.DEEP) or fam[1] >= 23, (G.family_id(fam), shape, is_sw, call)
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


DEEP_FAMS = [f for f in G.FAMILIES if f[1] == G.DEEP]


def _nw_band_of(c, k):
    """tests/test_gpu_magnitude.py's nw_band_of: the three bands per pair of its banded sections."""
    bands = G.nw_bands(c.shape, c.kind) if c.kind in ("gapb", "gapa", "both") else [(0, True), (1, True), (3, True)]
    return bands[k % len(bands)][0]


def test_the_families_that_run_under_nw_alone():
    assert {f[0] for f in G.FAMILIES if G.nw_only(f) and f[1] != G.DEEP} == set(G.FLOOR_BASES)
    assert [f[0] for f in DEEP_FAMS] == list(G.DEEP_BASES) and len(DEEP_FAMS) >= 4
    assert not {"nomismatch", "floor_mm"} & set(G.DEEP_BASES)      # the align walker's floor stepping under no_mismatches
    assert all(c.is_sw == 0 for f in G.FAMILIES if G.nw_only(f) for c in G.cases_of(fam=f))
    assert all({c.is_sw for c in G.cases_of(fam=f)} == {0, 1} for f in G.FAMILIES if not G.nw_only(f))


@pytest.mark.parametrize("fam", DEEP_FAMS, ids=G.family_id)
def test_deep_families_hold_real_scores_below_half_of_int32_min(fam):
    """Every deep case is defined upstream (all sums inside int32).  Some group that the score family admits has a pair whose
    global score lies below -2^30; some group that the banded calls admit has a pair whose banded end value lies below -2^30
    AND which the oracle walks inside its band (bandnwstatlib.want): an alignment, where the end value alone says there is
    none.  All of them above the floor, which stands within the largest |penalty| of INT32_MIN."""
    scores, banded = [], []
    for _, shape, is_sw, cs in G.groups(fam):
        assert not is_sw
        la, lb = G.group_lengths(cs)
        for c in cs:
            e = G.exact(c)
            assert e.fits_int32(), (c.id, e.lo, e.hi)
        if G.admitted(cs[0].spec, la, lb, "score"):
            for c in cs:
                rc, s, ra, rb = O.oracle_nw(c.osc(), c.a, c.b)
                assert rc == 0, c.id
                if s < -2 ** 30:
                    assert s > G.exact(c).floor, (c.id, s)
                    scores.append((c.id, s))
        if G.admitted(cs[0].spec, la, lb, "band"):
            for c in cs:
                for w in sorted({_nw_band_of(c, k) for k in range(3)}):
                    three = BN.want(c.osc(), c.a, c.b, w)
                    if three is not None and three[0] < -2 ** 30:
                        assert BN.below_half(c.osc(), c.a, c.b, w) and three[0] > G.exact(c).floor
                        banded.append((c.id, w, three))
    print(f"{G.family_id(fam)}: {len(scores)} admitted global scores below -2^30, lowest {min(s for _, s in scores)}; "
          f"{len(banded)} admitted banded end values below -2^30 that the oracle walks, e.g. {banded[0]}")
    assert scores and banded


# the calls of tests/test_gpu_magnitude.py's sections G and H: (name, NW | SW, the class of call whose admission rule it
# follows, whether it takes at most 512 diagonals)
NEW_CALLS = (("nw_stats", 0, "score", False), ("nw_stats_cross", 0, "score", False), ("sw_stats", 1, "score", False),
             ("sw_stats_cross", 1, "score", False), ("sw_span_cross", 1, "score", False), ("sw_span_search", 1, "score", False),
             ("nw_stats_banded", 0, "band", True), ("sw_stats_banded", 1, "band", True), ("nw_stats_banded_wide", 0, "band", False),
             ("sw_stats_banded_wide", 1, "band", False), ("sw_span_banded_wide", 1, "band", False))


def test_every_statistics_span_and_set_call_meets_both_sides_of_the_bound():
    """Across the matrix each of the eleven calls meets at least one group the documented rule admits and at least one it
    refuses, under the class of call it uses -- the score family's for the unbanded calls and the calls over sets (the
    longest query and the longest target are the group's longest seq_a and seq_b), the banded calls' for the rest.  The narrow
    banded calls count only the groups whose three band lists stay within their 512 diagonals (a wider band is refused for
    its width before the scoring is looked at)."""
    sides = {name: [0, 0] for name, *_ in NEW_CALLS}
    for fam, shape, is_sw, cs in G.groups():
        la, lb = G.group_lengths(cs)
        if is_sw:
            width = 12                                              # the SW band lists are at most 12 diagonals wide
        else:
            width = max(BL.width_of(len(c.a), len(c.b), _nw_band_of(c, k)) for c in cs for k in range(3))
        for name, sw, call, narrow in NEW_CALLS:
            if sw == is_sw and not (narrow and width > 512):
                sides[name][not G.admitted(cs[0].spec, la, lb, call)] += 1
    print(sides)
    assert all(adm > 0 and ref > 0 for adm, ref in sides.values()), sides


def test_the_mark_rule_and_the_value_rule_agree_on_the_banded_statistics_tests_lists():
    """seqalign_nw_stats_banded(_wide) decide "no alignment inside the band" by the sticky mark, which is bandnwstatlib.want's
    rule (the oracle's walk); they decided by the end value before (below_half).  On every case list of the banded NW
    statistics tests on which a pair may lose its alignment -- the 32 flag batches of the narrow file, the wide file's 32
    definition cases, the four row-flag lists at width 385, the whole tie batches under every band, the long pairs of the wide
    argument, and the pairs of both files' error tests under their strict table scoring -- the two rules name the same pairs,
    so nothing those tests assert has changed.  The GPU files take these lists from the same library functions.  (The small
    pairs: test_nw_stats_banded_argument_cpu.py and its wide sibling hold mark, value and want together pair by pair; every
    other list of the GPU files runs under a scoring that forbids no move and asserts that no pair is lost.)"""
    import itertools

    import bandnwstatwidelib as BW
    import bandspanlib as BSP
    import seqalign_amd as S
    import statlib as ST
    n = lost = 0

    def agree(osc, a, b, w):
        nonlocal n, lost
        none = BN.want(osc, a, b, w) is None
        assert none == BN.below_half(osc, a, b, w), (a, b, w)
        n += 1
        lost += none
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = O.build_scoring(spec, "oracle")
        alpha = b"ACGTacgt" + (b"N" if spec["wildcards"] else b"")
        for a, b, w in BN.flag_pairs(idx, flags, alpha) + BW.long_pairs(700 + idx, 4, b"ACac" + alpha[8:]):
            agree(osc, a, b, w)
    cases = BW.definition_cases()
    assert len(cases) == 32 and all(len(triples) == 8 for _, triples in cases)
    for init, triples in cases:
        osc = O.build_scoring({"init": init}, "oracle")
        for a, b, w in triples:
            agree(osc, a, b, w)
    for flag in BN.ROW_FLAGS:
        osc = O.build_scoring(ST.init_spec([1, -2, -4, -1], **{flag: 1}), "oracle")
        for a, b, w in BN.row_flag_triples(flag):
            agree(osc, a, b, w)
    for name in ST.TIE_SCORINGS:
        osc = O.build_scoring(ST.init_spec(ST.TIE_SCORINGS[name]), "oracle")
        for width in BN.TIE_WIDTHS:
            for a, b in BN.tie_batch(name, width):
                for w in BN.TIE_BANDS:
                    agree(osc, a, b, w)
    # the error tests of both files: a table scoring that forbids mismatches and both kinds of gap
    strict = S.make_scoring({"preset": "DNA_hybridization", "flags": {"no_mismatches": True, "no_gaps_in_a": True, "no_gaps_in_b": True}})
    ostrict = O.Scoring.from_buffer_copy(bytes(strict))
    before = lost
    for length, at in ((120, 60), (200, 160)):
        same, changed = BN.bandless_pair(length, at)
        agree(ostrict, same, same, 8)
        agree(ostrict, same, changed, 8)
    assert lost - before == 2
    print(f"{n} pairs, {lost} without an alignment inside their band under both rules")
    assert lost >= 40


def _fuzz_calls():
    tools = Path(__file__).resolve().parent.parent / "seq-align_amd" / "tools"
    spec = importlib.util.spec_from_file_location("dry_fuzz_calls", tools / "fuzz_calls.py")
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def test_the_fuzzers_copy_of_the_floor_walk_rule_is_the_librarys():
    """seq-align_amd/tools/fuzz_calls.py states walked_along_the_floor for itself (it takes only bandlib and statlib from the
    test helpers).  On the small pairs of the 32 flag combinations, where the family occurs, both copies say the same of every
    walk the oracle completes."""
    import itertools

    import bandspanlib as BSP
    fz, n, along = _fuzz_calls(), 0, 0
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = BSP.flag_scoring(idx, flags)
        osc = O.build_scoring(spec, "oracle")
        for a, b, w in BN.small_pairs(600 + idx, 60, b"ACac" + (b"N" if spec["wildcards"] else b"")):
            walked = BL.expected(osc, a, b, w)
            if walked is not None:
                mine, theirs = BN.walked_along_the_floor(osc, a, b, w, *walked[1:]), fz.walked_along_the_floor(osc, a, b, w, *walked[1:])
                assert mine == theirs, (flags, a, b, w)
                n += 1
                along += mine
    print(f"{n} walks, {along} of them along the floor")
    assert along >= 5, along


def test_fuzzer_scale_redraws_stay_under_one_trial_in_four():
    """seq-align_amd/tools/fuzz_calls.py with scale = 2^23, drawing only (no device): over 200 trials of the seeds the soak
    slice uses, at most one trial in four redraws its factor, and the default scale of 1 draws no factor at all."""
    fz = _fuzz_calls()
    for seed in (20261019, 3):
        r = fz.run(seconds=120.0, seed=seed, max_trials=100, scale=1 << 23, dry=True)
        assert r["trials"] == 100 and 4 * r["redrawn_trials"] <= r["trials"], r
        print(f"seed {seed}: {r['redrawn_trials']} of {r['trials']} trials redrew their factor ({r['redraws']} redraws)")
    plain = fz.run(seconds=30.0, seed=20261018, max_trials=5, dry=True)
    assert plain["redraws"] == 0 and plain["trials"] == 5
