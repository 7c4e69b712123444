"""CPU tier: the argument that tests/test_gpu_gap_dense.py tests what it claims -- on the oracle alone (and on the compiled
reference, oracle/_ref, through orclib.ref_nw where it was built).

The direction-byte paths never write the three matrices, so a wrong bit in a direction byte shows only through a walk that
reads it.  A walk that stands in GAP_A and whose predecessor is GAP_B -- an insertion run followed at once by a deletion run in
the gapped strings, I->D -- reads bits no other walk reads (SA_LD_BM through local_depart, the TY fallback of the older byte),
and under [1,-2,-4,-1] and [2,-2,-2,-1] no optimal alignment contains one.  Here: every pair the GPU cases count on has its
I->D transitions under the scoring it runs with, none under the two standard scorings, never a D->I (alignment_reverse_move
tests GAP_A first, src/alignment.c:311-327), CIGARs that outgrow the strings' len_a + len_b + 1 -- and the host's plane
decoders (host/sa_moves.c) on exactly these alignments, a run boundary at every column of a 32- and a 64-column word.
"""
import ctypes as C

import numpy as np
import pytest

import denselib as D
import orclib as O
import seqalign_amd as S
from test_moves_cpu import planes_from_alignment

_NW = {}


def oracle_nw(scoring, a, b):
    key = (scoring, a, b)
    if key not in _NW:
        rc, s, ra, rb = O.oracle_nw(D.oracle_scoring(scoring), a, b)
        assert rc == 0
        _NW[key] = (s, ra, rb)
    return _NW[key]


@pytest.mark.parametrize("scoring", D.NW_SCORINGS)
def test_every_counted_nw_pair_has_its_transitions(scoring):
    """Every pair of every NW case, none left out: at least the shape's floor of I->D (8; 3 at 31 x 40) in the oracle's global
    alignment, no D->I; the same sequences under the two standard scorings: not one transition of either kind.  The compiled
    reference, where built, gives the same strings."""
    ref_sc = O.build_scoring(D.SCORINGS[scoring], "ref") if O.ref() is not None else None
    seen = set()
    for label, floor, pairs in D.counted_nw_cases(scoring):
        counts = []
        for a, b in dict.fromkeys(pairs):
            s, ra, rb = oracle_nw(scoring, a, b)
            n_id = D.count_id(ra, rb)
            assert n_id >= floor >= 3, (scoring, label, len(a), len(b), n_id)
            assert D.count_di(ra, rb) == 0, (scoring, label, a, b)
            counts.append(n_id)
            if ref_sc is not None and (len(a) + 1) * (len(b) + 1) <= 1 << 18 and (a, b) not in seen:
                assert O.ref_nw(ref_sc, a, b) == (s, ra, rb), (scoring, label, a, b)
            if (a, b) not in seen:
                for control in D.CONTROLS:
                    _, ca, cb = oracle_nw(control, a, b)
                    assert D.count_id(ca, cb) == 0 and D.count_di(ca, cb) == 0, (control, label, a, b)
            seen.add((a, b))
        print(f"{scoring} {label}: {len(pairs)} pairs ({len(counts)} distinct), I->D min {min(counts)} total {sum(counts)}")


@pytest.mark.parametrize("scoring", D.SW_SCORINGS)
def test_every_counted_sw_pair_has_its_transitions(scoring):
    """The SW cases: the floor holds in the FIRST hit of every pair, no hit of any pair has a D->I, and no hit of the same
    sequences under the two standard scorings has an I->D."""
    for label, floor, pairs in D.counted_sw_cases(scoring):
        counts = []
        for a, b in dict.fromkeys(pairs):
            rc, hits = O.oracle_sw(D.oracle_scoring(scoring), a, b, D.SW_MIN_SCORE, 8)
            assert rc == 0 and hits, (scoring, label, a, b)
            n_id = D.count_id(hits[0]["a"], hits[0]["b"])
            assert n_id >= floor >= 3, (scoring, label, len(a), len(b), n_id)
            assert all(D.count_di(h["a"], h["b"]) == 0 for h in hits), (scoring, label, a, b)
            counts.append(n_id)
            for control in D.CONTROLS:
                rc, chits = O.oracle_sw(D.oracle_scoring(control), a, b, D.SW_MIN_SCORE, 8)
                assert rc == 0 and all(D.count_id(h["a"], h["b"]) == 0 and D.count_di(h["a"], h["b"]) == 0 for h in chits), (control, label)
        print(f"{scoring} {label}: {len(pairs)} pairs ({len(counts)} distinct), first hit I->D min {min(counts)} total {sum(counts)}")


def test_uncounted_pairs_are_only_ever_added():
    """The substituted pairs guarantee nothing (at short or lopsided shapes some have no I->D at all), so no counted list may
    contain one -- and they do add transitions where they can."""
    for scoring in D.NW_SCORINGS:
        counted = {p for _, _, pairs in D.counted_nw_cases(scoring) for p in pairs}
        total = 0
        for shape in D.NW_SHAPES:
            for a, b in D.nw_extra(shape, scoring):
                assert (a, b) not in counted
                if (len(a) + 1) * (len(b) + 1) <= 1 << 18:
                    _, ra, rb = oracle_nw(scoring, a, b)
                    assert D.count_di(ra, rb) == 0
                    total += D.count_id(ra, rb)
        assert total > 0, scoring


def test_alternation_cigars_outgrow_the_strings():
    """(AC)^75 against (AG)^75: 1M1I1D x 75 = 450 bytes against len_a + len_b + 1 = 301 under [2,-9,0,-1]; the best local hit
    under [5,-10,0,-1] and [1,0,0,0] has 223 columns and a 446-byte CIGAR.  Every square alternation pair of the GPU cases with
    one match per period: longer than the strings' slot, within the header's worst case 2 (len_a + len_b) + 1."""
    a, b = b"AC" * 75, b"AG" * 75
    _, ra, rb = oracle_nw("cheap0", a, b)
    assert D.cigar(ra, rb, D.M) == "1M1I1D" * 75 and len(D.cigar(ra, rb, D.M)) == 450 > len(a) + len(b) + 1 == 301
    assert D.cigar(ra, rb, D.EQX) == "1=1I1D" * 75
    for scoring in ("swdense", "ties"):
        rc, hits = O.oracle_sw(D.oracle_scoring(scoring), a, b, D.SW_MIN_SCORE, 1)
        assert rc == 0 and len(hits[0]["a"]) == 223 and len(D.cigar(hits[0]["a"], hits[0]["b"])) == 446
    for scoring in D.NW_SCORINGS:
        if D.matches_of(scoring) != 1:
            continue
        for shape in ("150x150", "m250", "m500"):
            for a, b in D.nw_alternation(shape, scoring):
                _, ra, rb = oracle_nw(scoring, a, b)
                for fmt in (D.M, D.EQX):
                    n = len(D.cigar(ra, rb, fmt))
                    assert len(a) + len(b) + 1 < n <= 2 * (len(a) + len(b)) + 1, (scoring, shape, fmt, n)


def test_long_runs_and_staircases():
    """The long-runs pairs: an insertion run and a deletion run of >= 198 columns each, back to back, once; the staircases:
    len_a I then len_b D, nothing else."""
    import re
    for scoring in ("cheap0", "ties", "ext0"):
        for a, b in D.long_run_pairs():
            _, ra, rb = oracle_nw(scoring, a, b)
            o = D.ops(ra, rb)
            assert D.count_di(ra, rb) == 0
            if set(a).isdisjoint(b):
                assert o == "I" * len(a) + "D" * len(b), (scoring, D.cigar(ra, rb))
            else:
                meet = [m for m in re.finditer(r"(I+)(D+)", o) if len(m.group(1)) + len(m.group(2)) >= 200]
                assert len(meet) == 1, (scoring, D.cigar(ra, rb))
                runs = [len(r) for r in re.findall(r"I+|D+", o)]
                assert sorted(runs)[-2] >= 198, (scoring, D.cigar(ra, rb))


# ------------------------------------------------------------------ the plane decoders on these alignments ---

def _decoder_alignments():
    """(a, b, ra, rb) of dense NW alignments: the 150 x 150 cases of three scorings, ragged ones, a few long ones."""
    out = []
    for scoring in ("cheap0", "ties", "ext0"):
        pairs = D.nw_uniform("150x150", scoring)[:12] + D.nw_ragged("150x150", scoring)[:12] + D.nw_ragged("31x40", scoring)[:6]
        pairs += D.nw_uniform("m250", scoring)[:2] + D.nw_extra("191x150", scoring)[:2] + D.long_run_pairs()[:4]
        for a, b in pairs:
            _, ra, rb = oracle_nw(scoring, a, b)
            out.append((a, b, ra, rb))
    return out


def _boundaries(ra, rb):
    o = D.ops(ra, rb)
    return {c for c in range(1, len(o)) if o[c] != o[c - 1]}


def test_decoder_alignments_put_a_run_boundary_on_every_column_of_a_word():
    """What the 300 related pairs of test_moves_cpu.py do not give the encoders: a boundary between two runs at every column of a
    64-column step (and so of a 32-column word), counted from the walk's end as the planes are laid out, and I->D among them."""
    at, id_at = set(), set()
    for a, b, ra, rb in _decoder_alignments():
        o = D.ops(ra, rb)
        n = len(o)
        at |= {(n - c) % 64 for c in _boundaries(ra, rb)}
        id_at |= {(n - c) % 64 for c in range(1, n) if o[c - 1:c + 1] == "ID"}
    assert at == set(range(64)) and id_at == set(range(64))


@pytest.mark.parametrize("scalar", [0, 1])
def test_dense_nw_planes_expand_and_encode(scalar):
    """sa_expand_nw_moves (SIMD and scalar loops) and sa_cigar_nw_moves, both formats: length only, exact capacity, one byte short
    -> E_NOMEM with nothing written past the capacity."""
    lib = S.lib()
    lib.sa_moves_force_scalar(C.c_int(scalar))
    try:
        for a, b, ra, rb in _decoder_alignments():
            pa, pb, n_words, n_moves = planes_from_alignment(ra, rb, len(a), len(b), True)
            first = 32 * n_words - n_moves
            for plane in (pa, pb):                       # poison what the walk did not write
                plane[:first // 32] = 0xDEADBEEF
                if first % 32:
                    plane[first // 32] |= np.uint32((1 << (first % 32)) - 1)
            oa, ob, n = C.create_string_buffer(len(a) + len(b) + 1), C.create_string_buffer(len(a) + len(b) + 1), C.c_uint32(0)
            rc = lib.sa_expand_nw_moves(a, C.c_uint32(len(a)), b, C.c_uint32(len(b)), pa.ctypes.data_as(C.c_void_p),
                                        pb.ctypes.data_as(C.c_void_p), C.c_uint32(n_words), C.c_uint32(n_moves), oa, ob, C.byref(n))
            assert rc == 0 and (oa.value, ob.value, n.value) == (ra, rb, len(ra))
            for fmt, fold in ((1, 0), (2, 0), (2, 1)):
                want = D.cigar(ra, rb, fmt, bool(fold)).encode()
                ln, cols = C.c_uint32(0), C.c_uint32(0)
                args = (a, C.c_uint32(len(a)), b, C.c_uint32(len(b)), pa.ctypes.data_as(C.c_void_p), pb.ctypes.data_as(C.c_void_p),
                        C.c_uint32(n_words), C.c_uint32(n_moves), C.c_int(fmt), C.c_int(fold))
                assert lib.sa_cigar_nw_moves(*args, None, C.c_uint64(0), C.byref(ln), C.byref(cols)) == 0
                assert (ln.value, cols.value) == (len(want), len(ra))
                out = C.create_string_buffer(b"\xff" * (len(want) + 9), len(want) + 9)
                assert lib.sa_cigar_nw_moves(*args, out, C.c_uint64(len(want) + 1), C.byref(ln), C.byref(cols)) == 0
                assert out.raw[:len(want) + 1] == want + b"\0" and out.raw[len(want) + 1:] == b"\xff" * 8
                out = C.create_string_buffer(b"\xff" * (len(want) + 9), len(want) + 9)
                assert lib.sa_cigar_nw_moves(*args, out, C.c_uint64(len(want)), C.byref(ln), C.byref(cols)) == S.E_NOMEM
                assert out.raw[len(want):] == b"\xff" * 9
    finally:
        lib.sa_moves_force_scalar(C.c_int(0))


@pytest.mark.parametrize("scalar", [0, 1])
def test_dense_sw_planes_expand_and_encode(scalar):
    """sa_expand_sw_moves and sa_cigar_sw_moves on the dense local hits (up to 4 per pair), the same capacities."""
    lib = S.lib()
    lib.sa_moves_force_scalar(C.c_int(scalar))
    done = 0
    try:
        for scoring in D.SW_SCORINGS:
            pairs = D.sw_uniform("150x150", scoring)[:10] + D.sw_ragged("191x150", scoring)[:6] + D.sw_planted_twice(scoring)[:6]
            for a, b in pairs:
                rc, hits = O.oracle_sw(D.oracle_scoring(scoring), a, b, D.SW_MIN_SCORE, 4)
                assert rc == 0 and hits
                for h in hits:
                    ra, rb = h["a"].encode(), h["b"].encode()
                    end_x, end_y = h["pos_a"] + h["len_a"], h["pos_b"] + h["len_b"]
                    where = [h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]]
                    pa, pb, n_words, n_moves = planes_from_alignment(ra, rb, len(a), len(b), False)
                    planes = (pa.ctypes.data_as(C.c_void_p), pb.ctypes.data_as(C.c_void_p), C.c_uint32(n_words), C.c_uint32(n_moves))
                    oa, ob, pos = C.create_string_buffer(len(a) + len(b) + 1), C.create_string_buffer(len(a) + len(b) + 1), (C.c_uint32 * 4)()
                    assert lib.sa_expand_sw_moves(a, b, C.c_uint32(end_x), C.c_uint32(end_y), *planes, oa, ob, pos) == 0
                    assert (oa.value, ob.value, list(pos)) == (ra, rb, where)
                    for fmt, fold in ((1, 0), (2, 1)):
                        want = D.cigar(ra, rb, fmt, bool(fold)).encode()
                        for cap, code in ((len(want) + 1, 0), (len(want), S.E_NOMEM)):
                            out, pos, n = C.create_string_buffer(b"\xff" * (len(want) + 9), len(want) + 9), (C.c_uint32 * 4)(), C.c_uint32(0)
                            rc = lib.sa_cigar_sw_moves(a, b, C.c_uint32(end_x), C.c_uint32(end_y), *planes, C.c_int(fmt), C.c_int(fold),
                                                       out, C.c_uint64(cap), pos, C.byref(n))
                            assert rc == code and n.value == len(want) and list(pos) == where
                            assert out.raw[cap:] == b"\xff" * (len(want) + 9 - cap)
                            if code == 0:
                                assert out.raw[:cap] == want + b"\0"
                    done += 1
        assert done > 100
    finally:
        lib.sa_moves_force_scalar(C.c_int(0))
