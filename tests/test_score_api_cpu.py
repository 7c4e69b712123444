"""CPU tier: the score-only calls' surface -- exported symbols, kernel kind names, argument checks of the C calls and of
the Python wrappers, all without a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_nw_score_batch", "seqalign_sw_score_batch", "seqalign_nw_score_batch_multi",
           "seqalign_sw_score_batch_multi", "seqalign_score_time_ms"]


def test_score_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)


def test_score_kernel_kinds_are_named():
    names = [S.lib().seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX)]
    assert b"score_rows" in names and b"score_strips" in names
    assert names.index(b"score_strips") == names.index(b"score_rows") + 1


def test_c_calls_refuse_null_arguments():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    batch = W.from_pairs([(b"ACGT", b"ACG")])
    d = S.batch_desc(batch)
    score, ea, eb = np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    null = C.c_void_p(0)
    assert lib.seqalign_nw_score_batch(null, C.byref(d), C.byref(sc), S._ptr(score)) == S.E_ARG
    assert lib.seqalign_sw_score_batch(null, C.byref(d), C.byref(sc), S._ptr(score), S._ptr(ea), S._ptr(eb)) == S.E_ARG
    assert lib.seqalign_nw_score_batch_multi(null, C.c_int(1), C.byref(d), C.byref(sc), S._ptr(score)) == S.E_ARG
    assert lib.seqalign_sw_score_batch_multi(null, C.c_int(1), C.byref(d), C.byref(sc), S._ptr(score), S._ptr(ea),
                                             S._ptr(eb)) == S.E_ARG
    assert lib.seqalign_score_time_ms(null, C.byref(d), C.byref(sc), C.c_int(0), C.c_int(1), null) == S.E_ARG


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_score", "sw_score"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    good = W.from_pairs([(b"ACGT", b"ACG"), (b"", b"T")])
    fn = getattr(ctx, call)
    with pytest.raises(S.SeqAlignError) as e:
        fn(good, sc)                                   # a valid batch reaches the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_" in str(e.value)
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
