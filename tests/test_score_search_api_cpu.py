"""CPU tier: the top-k score search's surface -- exported symbols, the kernel kind name, argument checks of the C calls and
of the Python wrappers, all without a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_nw_score_search", "seqalign_sw_score_search", "seqalign_nw_score_search_multi",
           "seqalign_sw_score_search_multi"]


def test_search_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)


def test_select_kernel_kind_is_named_after_the_cross_kernel():
    names = [S.lib().seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX)]
    assert b"score_select" in names
    assert names.index(b"score_select") == names.index(b"score_cross") + 1


def test_hit_dtype_is_the_c_struct():
    assert S.SEARCH_HIT.itemsize == 16 and S.SEARCH_HIT.names == ("target", "score", "end_a", "end_b")
    assert S.SEARCH_MAX_K == 1024 and S.INT32_MIN == -2**31


def _sets():
    return W.seqset_from([b"ACGT", b"", b"GATTACA"]), W.seqset_from([b"ACG", b"TTT"])


def _calls(lib):
    """(name, call(ctx_or_list, q, t, sc, k, hits, n_hits)) for the four C calls; the _multi ones get a one-entry list."""
    def single(fn):
        return lambda c, q, t, sc, k, h, n: fn(c, q, t, sc, C.c_uint32(k), C.c_int32(0), h, n)

    def multi(fn):
        return lambda c, q, t, sc, k, h, n: fn((C.c_void_p * 1)(c.value) if c.value else C.c_void_p(0), C.c_int(1), q, t,
                                               sc, C.c_uint32(k), C.c_int32(0), h, n)
    return [("nw", single(lib.seqalign_nw_score_search)), ("sw", single(lib.seqalign_sw_score_search)),
            ("nw_multi", multi(lib.seqalign_nw_score_search_multi)), ("sw_multi", multi(lib.seqalign_sw_score_search_multi))]


def test_c_calls_refuse_null_arguments():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    dq, dt = S.seqset_desc(q), S.seqset_desc(t)
    hits, n_hits = np.zeros((3, 4), S.SEARCH_HIT), np.zeros(3, np.uint32)
    null, fake = C.c_void_p(0), C.c_void_p(1)
    for name, call in _calls(lib):
        assert call(null, C.byref(dq), C.byref(dt), C.byref(sc), 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), C.byref(dt), null, 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), C.byref(dt), C.byref(sc), 4, null, S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), C.byref(dt), C.byref(sc), 4, S._ptr(hits), null) == S.E_ARG, name
        assert call(fake, null, C.byref(dt), C.byref(sc), 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), null, C.byref(sc), 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name


def test_c_calls_check_k_and_sizes_before_reading_anything():
    """k = 0, k = 1025, n_targets > UINT32_MAX and n_queries x n_targets past 2^64 are SEQALIGN_E_ARG with sets and outputs
    whose arrays point nowhere, before the context is used (the handle is not a context)."""
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    fake = C.c_void_p(1)                       # never dereferenced: every case below fails first
    nowhere = C.c_void_p(8)
    small = S.SeqSetDesc(3, 1, 0, 1, 1)        # non-NULL arrays that point nowhere
    many_t = S.SeqSetDesc((1 << 32) + 5, 1, 0, 1, 1)
    huge = S.SeqSetDesc(1 << 33, 1, 0, 1, 1)
    for name, call in _calls(lib):
        for k in (0, 1025, 1 << 31):
            assert call(fake, C.byref(small), C.byref(small), C.byref(sc), k, nowhere, nowhere) == S.E_ARG, (name, k)
            assert "k must be" in lib.seqalign_last_error().decode()
        assert call(fake, C.byref(small), C.byref(many_t), C.byref(sc), 7, nowhere, nowhere) == S.E_ARG, name
        assert "UINT32_MAX" in lib.seqalign_last_error().decode()
        assert call(fake, C.byref(huge), C.byref(huge), C.byref(sc), 7, nowhere, nowhere) == S.E_ARG, name
        assert "overflow" in lib.seqalign_last_error().decode()
        no_arrays = S.SeqSetDesc(3, 1, 0, 0, 0)
        assert call(fake, C.byref(no_arrays), C.byref(small), C.byref(sc), 7, nowhere, nowhere) == S.E_ARG, name


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_score_search", "sw_score_search"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    fn = getattr(ctx, call)
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, sc, 3)                                # valid arguments reach the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_" in str(e.value) and "search" in str(e.value)
    for k in (0, 1025, -1, 2.0, "3", True, None):
        with pytest.raises(S.SeqAlignError) as e:
            fn(q, t, sc, k)
        assert e.value.code == S.E_ARG and "k must be" in str(e.value), k
    for m in (2**31, -2**31 - 1, 1.5, None):
        with pytest.raises(S.SeqAlignError) as e:
            fn(q, t, sc, 3, min_score=m)
        assert e.value.code == S.E_ARG and "min_score" in str(e.value), m
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, {"preset": "default"}, 3)             # not a scoring_t
    assert e.value.code == S.E_ARG
    outside = W.SeqSet(t.arena, t.off.copy(), t.len.copy())
    outside.off[1] = np.uint64(t.arena.nbytes - 1)
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, outside, sc, 3)                          # a sequence past its arena's end
    assert e.value.code == S.E_ARG and "outside" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        fn(W.SeqSet(q.arena, q.off.astype(np.int64), q.len), t, sc, 3)
    assert e.value.code == S.E_ARG and "queries." in str(e.value)
    with pytest.raises(S.SeqAlignError):
        fn(q, W.from_pairs([(b"A", b"C")]), sc, 3)     # a Batch is not a set
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, sc, np.int64(3), min_score=np.int32(-5))   # numpy integers are accepted
    assert "seqalign_" in str(e.value)
