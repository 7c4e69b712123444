"""CPU tier: the NW statistics calls' surface -- exported and declared symbols, the unchanged kernel kind tables, argument
checks of the C calls before any device is looked for, and of the Python wrappers."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_nw_stats_batch", "seqalign_nw_stats_batch_multi", "seqalign_nw_stats_time_ms", "seqalign_nw_stats_cross"]


def test_stats_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)
    header = (S.LIB_PATH.parent.parent.parent / "include" / "seqalign_hip.h").read_text()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert all(callable(getattr(S.Context, f)) for f in ("nw_stats", "nw_stats_time_ms", "nw_stats_cross"))


def test_kind_tables_are_unchanged():
    """The calls add no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def test_c_calls_refuse_bad_arguments_before_any_device():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"A", b"")])
    d = S.batch_desc(b)
    score, m, mm = np.zeros(2, np.int32), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    ms = np.zeros(1, np.float32)
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    P = S._ptr
    args = [fake, C.byref(d), C.byref(sc), P(score), P(m), P(mm)]
    for k in range(len(args)):
        bad = list(args)
        bad[k] = null
        assert lib.seqalign_nw_stats_batch(*bad) == S.E_ARG, k
    ctxs = (C.c_void_p * 1)(fake.value)
    margs = [ctxs, C.c_int(1)] + args[1:]
    for k in (0, 2, 3, 4, 5, 6):
        bad = list(margs)
        bad[k] = null
        assert lib.seqalign_nw_stats_batch_multi(*bad) == S.E_ARG, k
    assert lib.seqalign_nw_stats_batch_multi(ctxs, C.c_int(0), *args[1:]) == S.E_ARG
    targs = [fake, C.byref(d), C.byref(sc), C.c_int(1), P(ms)]
    for k in (0, 1, 2, 4):
        bad = list(targs)
        bad[k] = null
        assert lib.seqalign_nw_stats_time_ms(*bad) == S.E_ARG, k
    assert lib.seqalign_nw_stats_time_ms(fake, C.byref(d), C.byref(sc), C.c_int(0), P(ms)) == S.E_ARG
    # a batch whose arrays are missing
    unreadable = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert lib.seqalign_nw_stats_batch(fake, C.byref(unreadable), C.byref(sc), P(score), P(m), P(mm)) == S.E_ARG
    assert lib.seqalign_nw_stats_batch_multi(ctxs, C.c_int(1), C.byref(unreadable), C.byref(sc), P(score), P(m), P(mm)) == S.E_ARG
    assert lib.seqalign_nw_stats_time_ms(fake, C.byref(unreadable), C.byref(sc), C.c_int(1), P(ms)) == S.E_ARG
    # the cross call: its sets
    q = W.seqset_from([b"ACGT", b"AC"])
    dq = S.seqset_desc(q)
    cargs = [fake, C.byref(dq), C.byref(dq), C.byref(sc), P(score), P(m), P(mm)]
    for k in range(len(cargs)):
        bad = list(cargs)
        bad[k] = null
        assert lib.seqalign_nw_stats_cross(*bad) == S.E_ARG, k
    no_arrays = S.SeqSetDesc(3, q.arena.ctypes.data, q.arena.nbytes, 0, 0)
    assert lib.seqalign_nw_stats_cross(fake, C.byref(no_arrays), C.byref(dq), C.byref(sc), P(score), P(m), P(mm)) == S.E_ARG
    huge = S.SeqSetDesc(1 << 33, 1, 0, 1, 1)   # non-NULL arrays that point nowhere: the size check comes first
    assert lib.seqalign_nw_stats_cross(fake, C.byref(huge), C.byref(huge), C.byref(sc), P(score), P(m), P(mm)) == S.E_ARG
    assert "overflow" in lib.seqalign_last_error().decode()


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_stats", "nw_stats_time_ms"])
def test_batch_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    good = W.from_pairs([(b"ACGT", b"ACG"), (b"", b"T")])
    fn = getattr(ctx, call)
    with pytest.raises(S.SeqAlignError) as e:
        fn(good, sc)                                   # a valid batch reaches the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_nw_stats" in str(e.value)
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
    if call == "nw_stats_time_ms":
        with pytest.raises(S.SeqAlignError) as e:
            fn(good, sc, repeats=0)
        assert e.value.code == S.E_ARG and "repeats" in str(e.value)


def test_cross_wrapper_checks_its_arguments():
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    q, t = W.seqset_from([b"ACGT", b"AC"]), W.seqset_from([b"ACG", b"", b"T"])
    with pytest.raises(S.SeqAlignError) as e:
        ctx.nw_stats_cross(q, t, sc)                   # valid sets reach the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_nw_stats_cross" in str(e.value)
    with pytest.raises(S.SeqAlignError):
        ctx.nw_stats_cross(q, t, {"preset": "default"})
    for wrong in (W.SeqSet(q.arena, q.off.astype(np.int64), q.len), W.SeqSet(q.arena, q.off[:1], q.len), object()):
        with pytest.raises(S.SeqAlignError) as e:
            ctx.nw_stats_cross(wrong, t, sc)
        assert e.value.code == S.E_ARG
        with pytest.raises(S.SeqAlignError):
            ctx.nw_stats_cross(q, wrong, sc)
