"""CPU tier: the SW hit-span call's surface -- exported symbols, the unchanged kernel kind tables, argument checks of the C
calls and of the Python wrappers, all without a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_sw_span_batch", "seqalign_sw_span_batch_multi", "seqalign_sw_span_time_ms"]


def test_span_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)
    assert callable(S.Context.sw_span) and callable(S.Context.sw_span_time_ms)


def test_kind_tables_are_unchanged():
    """The call adds no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    assert b"score_rows" in first and first.index(b"score_strips") == first.index(b"score_rows") + 1
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def test_c_calls_refuse_null_arguments():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    batch = W.from_pairs([(b"ACGT", b"ACG")])
    d = S.batch_desc(batch)
    score = np.zeros(1, np.int32)
    u = [np.zeros(1, np.uint32) for _ in range(4)]
    null = C.c_void_p(0)
    outs = [S._ptr(score)] + [S._ptr(x) for x in u]
    assert lib.seqalign_sw_span_batch(null, C.byref(d), C.byref(sc), *outs) == S.E_ARG
    assert lib.seqalign_sw_span_batch_multi(null, C.c_int(1), C.byref(d), C.byref(sc), *outs) == S.E_ARG
    assert lib.seqalign_sw_span_batch_multi(null, C.c_int(0), C.byref(d), C.byref(sc), *outs) == S.E_ARG
    assert lib.seqalign_sw_span_time_ms(null, C.byref(d), C.byref(sc), C.c_int(1), null) == S.E_ARG
    ms = np.zeros(1, np.float32)
    assert lib.seqalign_sw_span_time_ms(null, C.byref(d), C.byref(sc), C.c_int(1), S._ptr(ms)) == S.E_ARG


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["sw_span", "sw_span_time_ms"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    good = W.from_pairs([(b"ACGT", b"ACG"), (b"", b"T")])
    fn = getattr(ctx, call)
    with pytest.raises(S.SeqAlignError) as e:
        fn(good, sc)                                   # a valid batch reaches the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_sw_span" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        fn(good, {"preset": "default"})                # not a scoring_t
    assert e.value.code == S.E_ARG
    outside = W.Batch(good.arena, good.off_a.copy(), good.len_a.copy(), good.off_b.copy(), good.len_b.copy())
    outside.off_b[0] = np.uint64(good.arena.nbytes)
    with pytest.raises(S.SeqAlignError) as e:
        fn(outside, sc)                                # a sequence past the arena's end
    assert e.value.code == S.E_ARG and "outside" in str(e.value)
    wrong = W.Batch(good.arena, good.off_a.astype(np.int64), good.len_a, good.off_b, good.len_b)
    with pytest.raises(S.SeqAlignError) as e:
        fn(wrong, sc)                                  # descriptor arrays of the wrong type
    assert e.value.code == S.E_ARG and "off_a" in str(e.value)
    with pytest.raises(S.SeqAlignError):
        fn(object(), sc)
    if call == "sw_span_time_ms":
        with pytest.raises(S.SeqAlignError) as e:
            fn(good, sc, repeats=0)
        assert e.value.code == S.E_ARG and "repeats" in str(e.value)
