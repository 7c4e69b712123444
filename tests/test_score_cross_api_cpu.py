"""CPU tier: the score-matrix calls' surface -- exported symbols, the kernel kind name, argument checks of the C calls and of
the Python wrappers, the set helpers of workloads, all without a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_nw_score_cross", "seqalign_sw_score_cross", "seqalign_nw_score_cross_multi",
           "seqalign_sw_score_cross_multi"]


def test_cross_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)


def test_cross_kernel_kind_is_named_after_the_strips():
    names = [S.lib().seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX)]
    assert b"score_cross" in names
    assert names.index(b"score_cross") == names.index(b"score_strips") + 1


def _sets():
    return W.seqset_from([b"ACGT", b"", b"GATTACA"]), W.seqset_from([b"ACG", b"TTT"])


def test_c_calls_refuse_null_arguments():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    dq, dt = S.seqset_desc(q), S.seqset_desc(t)
    score, ea, eb = (np.zeros(6, np.int32), np.zeros(6, np.uint32), np.zeros(6, np.uint32))
    null = C.c_void_p(0)
    assert lib.seqalign_nw_score_cross(null, C.byref(dq), C.byref(dt), C.byref(sc), S._ptr(score)) == S.E_ARG
    assert lib.seqalign_sw_score_cross(null, C.byref(dq), C.byref(dt), C.byref(sc), S._ptr(score), S._ptr(ea),
                                       S._ptr(eb)) == S.E_ARG
    assert lib.seqalign_nw_score_cross_multi(null, C.c_int(1), C.byref(dq), C.byref(dt), C.byref(sc), S._ptr(score)) == S.E_ARG
    assert lib.seqalign_sw_score_cross_multi(null, C.c_int(1), C.byref(dq), C.byref(dt), C.byref(sc), S._ptr(score),
                                             S._ptr(ea), S._ptr(eb)) == S.E_ARG


def test_c_calls_check_sets_and_size_before_reading_them():
    """NULL sets, a set of n > 0 without its arrays, and n_queries x n_targets past 2^64 are SEQALIGN_E_ARG -- the last
    with array pointers that point nowhere, so nothing may read them -- all before the context is used (the handle is not a
    context)."""
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    score, ea, eb = np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    q, t = _sets()
    dq, dt = S.seqset_desc(q), S.seqset_desc(t)
    fake = C.c_void_p(1)   # never dereferenced: every case below fails on the sets
    no_arrays = S.SeqSetDesc(3, q.arena.ctypes.data, q.arena.nbytes, 0, 0)
    for a, b in ((None, dt), (dq, None), (no_arrays, dt), (dq, no_arrays)):
        pa = C.byref(a) if a is not None else C.c_void_p(0)
        pb = C.byref(b) if b is not None else C.c_void_p(0)
        assert lib.seqalign_nw_score_cross(fake, pa, pb, C.byref(sc), S._ptr(score)) == S.E_ARG
        assert lib.seqalign_sw_score_cross(fake, pa, pb, C.byref(sc), S._ptr(score), S._ptr(ea), S._ptr(eb)) == S.E_ARG
    huge = S.SeqSetDesc(1 << 33, 1, 0, 1, 1)   # non-NULL arrays that point nowhere: the size check comes first
    assert lib.seqalign_nw_score_cross(fake, C.byref(huge), C.byref(huge), C.byref(sc), S._ptr(score)) == S.E_ARG
    assert "overflow" in lib.seqalign_last_error().decode()
    ctxs = (C.c_void_p * 1)(fake.value)
    assert lib.seqalign_sw_score_cross_multi(ctxs, C.c_int(1), C.byref(huge), C.byref(huge), C.byref(sc), S._ptr(score),
                                             S._ptr(ea), S._ptr(eb)) == S.E_ARG


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_score_cross", "sw_score_cross"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    fn = getattr(ctx, call)
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, sc)                                   # valid sets reach the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, {"preset": "default"})                # not a scoring_t
    assert e.value.code == S.E_ARG
    outside = W.SeqSet(t.arena, t.off.copy(), t.len.copy())
    outside.off[1] = np.uint64(t.arena.nbytes - 1)
    for a, b, which in ((q, outside, "targets"), (outside, t, "queries")):
        with pytest.raises(S.SeqAlignError) as e:
            fn(a, b, sc)                               # a sequence past its arena's end
        assert e.value.code == S.E_ARG and "outside" in str(e.value) and which in str(e.value)
    for wrong in (W.SeqSet(q.arena, q.off.astype(np.int64), q.len), W.SeqSet(q.arena, q.off, q.len.astype(np.uint64)),
                  W.SeqSet(q.arena, q.off[:2], q.len), W.SeqSet(q.arena.astype(np.int8), q.off, q.len)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(wrong, t, sc)                           # arrays of the wrong type or length
        assert e.value.code == S.E_ARG and "queries." in str(e.value)
    with pytest.raises(S.SeqAlignError):
        fn(object(), t, sc)
    with pytest.raises(S.SeqAlignError):
        fn(q, W.from_pairs([(b"A", b"C")]), sc)        # a Batch is not a set


def test_set_helpers():
    s = W.seqset_from([b"ACGT", b"", b"GG"])
    assert s.n_seqs == 3 and [s.seq(i) for i in range(3)] == [b"ACGT", b"", b"GG"]
    assert s.off.dtype == np.uint64 and s.len.dtype == np.uint32
    r1, r2 = W.random_set(50, 7, 3, 40, bytes(W.AMINO20)), W.random_set(50, 7, 3, 40, bytes(W.AMINO20))
    assert np.array_equal(r1.arena, r2.arena) and np.array_equal(r1.len, r2.len)
    assert int(r1.len.min()) >= 3 and int(r1.len.max()) <= 40
    assert set(r1.arena[:-1].tobytes()) <= set(bytes(W.AMINO20))
    b = W.cross_batch(s, r1)
    assert b.n_pairs == 3 * 50
    for q in range(3):
        for t in (0, 17, 49):
            p = q * 50 + t
            assert b.seq_a(p) == s.seq(q) and b.seq_b(p) == r1.seq(t)
