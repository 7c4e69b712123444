"""CPU tier: the surface of the SW hit-span calls over two sets (seqalign_sw_span_cross, seqalign_sw_span_search and their
_multi forms) -- exported symbols, the hit record, the unchanged kernel kind tables, argument checks of the C calls and of the
Python wrappers, all without a device."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_sw_span_cross", "seqalign_sw_span_cross_multi", "seqalign_sw_span_search", "seqalign_sw_span_search_multi"]


def test_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)
    header = (S.REPO_ROOT / "include" / "seqalign_hip.h").read_text()
    for name in SYMBOLS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert "seqalign_span_hit_t" in header
    assert callable(S.Context.sw_span_cross) and callable(S.Context.sw_span_search)


def test_hit_dtype_is_the_c_struct():
    assert S.SPAN_HIT.itemsize == 24
    assert S.SPAN_HIT.names == ("target", "score", "pos_a", "pos_b", "len_a", "len_b")
    assert [S.SPAN_HIT.fields[n][1] for n in S.SPAN_HIT.names] == [0, 4, 8, 12, 16, 20]


def test_kind_tables_are_unchanged():
    """The calls add no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    assert b"score_rows" in first and first.index(b"score_strips") == first.index(b"score_rows") + 1
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def _sets():
    return W.seqset_from([b"ACGT", b"", b"GATTACA"]), W.seqset_from([b"ACG", b"TTT"])


def _ctx_arg(c, multi):
    """The first arguments of a call: the handle, or for a _multi call a one-entry list of it (NULL stays NULL) and its length."""
    if not multi:
        return (c,)
    return ((C.c_void_p * 1)(c.value) if c.value else C.c_void_p(0), C.c_int(1))


def _cross_calls(lib):
    return [("cross", lambda c, *rest: lib.seqalign_sw_span_cross(*_ctx_arg(c, False), *rest)),
            ("cross_multi", lambda c, *rest: lib.seqalign_sw_span_cross_multi(*_ctx_arg(c, True), *rest))]


def _search_calls(lib):
    def tail(q, t, sc, k, h, n):
        return (q, t, sc, C.c_uint32(k), C.c_int32(0), h, n)
    return [("search", lambda c, *a: lib.seqalign_sw_span_search(*_ctx_arg(c, False), *tail(*a))),
            ("search_multi", lambda c, *a: lib.seqalign_sw_span_search_multi(*_ctx_arg(c, True), *tail(*a)))]


def test_cross_calls_refuse_null_arguments():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    dq, dt = S.seqset_desc(q), S.seqset_desc(t)
    outs = [S._ptr(np.zeros((3, 2), np.int32))] + [S._ptr(np.zeros((3, 2), np.uint32)) for _ in range(4)]
    null, fake = C.c_void_p(0), C.c_void_p(1)     # fake: not a context, and never dereferenced -- every case fails first
    for name, call in _cross_calls(lib):
        assert call(null, C.byref(dq), C.byref(dt), C.byref(sc), *outs) == S.E_ARG, name
        assert call(fake, C.byref(dq), C.byref(dt), null, *outs) == S.E_ARG, name
        assert call(fake, null, C.byref(dt), C.byref(sc), *outs) == S.E_ARG, name
        assert call(fake, C.byref(dq), null, C.byref(sc), *outs) == S.E_ARG, name
        for i in range(5):
            assert call(fake, C.byref(dq), C.byref(dt), C.byref(sc), *[null if j == i else o for j, o in enumerate(outs)]) == S.E_ARG, (name, i)
    assert lib.seqalign_sw_span_cross_multi(C.c_void_p(0), C.c_int(0), C.byref(dq), C.byref(dt), C.byref(sc), *outs) == S.E_ARG


def test_search_calls_refuse_null_arguments():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    dq, dt = S.seqset_desc(q), S.seqset_desc(t)
    hits, n_hits = np.zeros((3, 4), S.SPAN_HIT), np.zeros(3, np.uint32)
    null, fake = C.c_void_p(0), C.c_void_p(1)
    for name, call in _search_calls(lib):
        assert call(null, C.byref(dq), C.byref(dt), C.byref(sc), 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), C.byref(dt), null, 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), C.byref(dt), C.byref(sc), 4, null, S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), C.byref(dt), C.byref(sc), 4, S._ptr(hits), null) == S.E_ARG, name
        assert call(fake, null, C.byref(dt), C.byref(sc), 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name
        assert call(fake, C.byref(dq), null, C.byref(sc), 4, S._ptr(hits), S._ptr(n_hits)) == S.E_ARG, name


def test_sizes_are_checked_before_anything_is_read():
    """k = 0, k = 1 025, n_targets > UINT32_MAX and n_queries x n_targets past 2^64 are SEQALIGN_E_ARG with sets and outputs
    whose arrays point nowhere, before the context is used (the handle is not a context)."""
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    fake, nowhere = C.c_void_p(1), C.c_void_p(8)
    small = S.SeqSetDesc(3, 1, 0, 1, 1)        # non-NULL arrays that point nowhere
    many_t = S.SeqSetDesc((1 << 32) + 5, 1, 0, 1, 1)
    huge = S.SeqSetDesc(1 << 33, 1, 0, 1, 1)
    no_arrays = S.SeqSetDesc(3, 1, 0, 0, 0)
    for name, call in _search_calls(lib):
        for k in (0, 1025, 1 << 31):
            assert call(fake, C.byref(small), C.byref(small), C.byref(sc), k, nowhere, nowhere) == S.E_ARG, (name, k)
            assert "k must be" in lib.seqalign_last_error().decode()
        assert call(fake, C.byref(small), C.byref(many_t), C.byref(sc), 7, nowhere, nowhere) == S.E_ARG, name
        assert "UINT32_MAX" in lib.seqalign_last_error().decode()
        assert call(fake, C.byref(huge), C.byref(huge), C.byref(sc), 7, nowhere, nowhere) == S.E_ARG, name
        assert "overflow" in lib.seqalign_last_error().decode()
        assert call(fake, C.byref(no_arrays), C.byref(small), C.byref(sc), 7, nowhere, nowhere) == S.E_ARG, name
    for name, call in _cross_calls(lib):
        outs = [nowhere] * 5
        assert call(fake, C.byref(huge), C.byref(huge), C.byref(sc), *outs) == S.E_ARG, name
        assert "overflow" in lib.seqalign_last_error().decode()
        assert call(fake, C.byref(no_arrays), C.byref(small), C.byref(sc), *outs) == S.E_ARG, name
        assert call(fake, C.byref(small), C.byref(no_arrays), C.byref(sc), *outs) == S.E_ARG, name


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


def test_python_cross_wrapper_checks_its_arguments():
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_span_cross(q, t, sc)                    # valid arguments reach the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_sw_span_cross" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_span_cross(q, t, {"preset": "default"})  # not a scoring_t
    assert e.value.code == S.E_ARG
    outside = W.SeqSet(t.arena, t.off.copy(), t.len.copy())
    outside.off[1] = np.uint64(t.arena.nbytes - 1)
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_span_cross(q, outside, sc)              # a sequence past its arena's end
    assert e.value.code == S.E_ARG and "outside" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_span_cross(W.SeqSet(q.arena, q.off.astype(np.int64), q.len), t, sc)
    assert e.value.code == S.E_ARG and "queries." in str(e.value)
    with pytest.raises(S.SeqAlignError):
        ctx.sw_span_cross(q, W.from_pairs([(b"A", b"C")]), sc)     # a Batch is not a set


def test_python_search_wrapper_checks_its_arguments():
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    q, t = _sets()
    fn = ctx.sw_span_search
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, sc, 3)
    assert e.value.code == S.E_ARG and "seqalign_sw_span_search" in str(e.value)
    for k in (0, 1025, -1, 2.0, "3", True, None):
        with pytest.raises(S.SeqAlignError) as e:
            fn(q, t, sc, k)
        assert e.value.code == S.E_ARG and "k must be" in str(e.value), k
    for m in (2**31, -2**31 - 1, 1.5, None):
        with pytest.raises(S.SeqAlignError) as e:
            fn(q, t, sc, 3, min_score=m)
        assert e.value.code == S.E_ARG and "min_score" in str(e.value), m
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, {"preset": "default"}, 3)
    assert e.value.code == S.E_ARG
    outside = W.SeqSet(t.arena, t.off.copy(), t.len.copy())
    outside.off[1] = np.uint64(t.arena.nbytes - 1)
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, outside, sc, 3)
    assert e.value.code == S.E_ARG and "outside" in str(e.value)
    with pytest.raises(S.SeqAlignError):
        fn(q, W.from_pairs([(b"A", b"C")]), sc, 3)
    with pytest.raises(S.SeqAlignError) as e:
        fn(q, t, sc, np.int64(3), min_score=np.int32(-5))   # numpy integers are accepted
    assert "seqalign_sw_span_search" in str(e.value)
