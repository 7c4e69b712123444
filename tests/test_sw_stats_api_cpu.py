"""CPU tier: the SW statistics calls' surface -- exported and declared symbols, the unchanged kernel kind tables, argument checks
of the C calls before any device is looked for (the length limit among them, in both orders), and of the Python wrappers."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_sw_stats_batch", "seqalign_sw_stats_batch_multi", "seqalign_sw_stats_time_ms", "seqalign_sw_stats_cross"]
MAX_LEN = 65535


def test_stats_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)
    header = (S.LIB_PATH.parent.parent.parent / "include" / "seqalign_hip.h").read_text()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"^#define SEQALIGN_SW_STATS_MAX_LEN 65535u$", header, re.M) and S.SW_STATS_MAX_LEN == MAX_LEN
    assert all(callable(getattr(S.Context, f)) for f in ("sw_stats", "sw_stats_time_ms", "sw_stats_cross"))


def test_kind_tables_are_unchanged():
    """The calls add no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def outputs(n):
    return [np.zeros(n, np.int32)] + [np.zeros(n, np.uint32) for _ in range(6)]


def test_c_calls_refuse_bad_arguments_before_any_device():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"A", b"")])
    d = S.batch_desc(b)
    out = [S._ptr(x) for x in outputs(4)]
    ms = np.zeros(1, np.float32)
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args = [fake, C.byref(d), C.byref(sc)] + out
    for k in range(len(args)):
        bad = list(args)
        bad[k] = null
        assert lib.seqalign_sw_stats_batch(*bad) == S.E_ARG, k
    ctxs = (C.c_void_p * 1)(fake.value)
    margs = [ctxs, C.c_int(1)] + args[1:]
    for k in [0] + list(range(2, len(margs))):
        bad = list(margs)
        bad[k] = null
        assert lib.seqalign_sw_stats_batch_multi(*bad) == S.E_ARG, k
    assert lib.seqalign_sw_stats_batch_multi(ctxs, C.c_int(0), *args[1:]) == S.E_ARG
    assert lib.seqalign_sw_stats_batch_multi((C.c_void_p * 2)(fake.value, 0), C.c_int(2), *args[1:]) == S.E_ARG
    targs = [fake, C.byref(d), C.byref(sc), C.c_int(1), S._ptr(ms)]
    for k in (0, 1, 2, 4):
        bad = list(targs)
        bad[k] = null
        assert lib.seqalign_sw_stats_time_ms(*bad) == S.E_ARG, k
    assert lib.seqalign_sw_stats_time_ms(fake, C.byref(d), C.byref(sc), C.c_int(0), S._ptr(ms)) == S.E_ARG
    empty = S.batch_desc(W.from_pairs([]))
    assert lib.seqalign_sw_stats_time_ms(fake, C.byref(empty), C.byref(sc), C.c_int(1), S._ptr(ms)) == S.E_ARG
    # a batch whose arrays are missing
    unreadable = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert lib.seqalign_sw_stats_batch(fake, C.byref(unreadable), C.byref(sc), *out) == S.E_ARG
    assert lib.seqalign_sw_stats_batch_multi(ctxs, C.c_int(1), C.byref(unreadable), C.byref(sc), *out) == S.E_ARG
    assert lib.seqalign_sw_stats_time_ms(fake, C.byref(unreadable), C.byref(sc), C.c_int(1), S._ptr(ms)) == S.E_ARG
    # the cross call: its sets
    q = W.seqset_from([b"ACGT", b"AC"])
    dq = S.seqset_desc(q)
    cargs = [fake, C.byref(dq), C.byref(dq), C.byref(sc)] + out
    for k in range(len(cargs)):
        bad = list(cargs)
        bad[k] = null
        assert lib.seqalign_sw_stats_cross(*bad) == S.E_ARG, k
    no_arrays = S.SeqSetDesc(3, q.arena.ctypes.data, q.arena.nbytes, 0, 0)
    assert lib.seqalign_sw_stats_cross(fake, C.byref(no_arrays), C.byref(dq), C.byref(sc), *out) == S.E_ARG
    huge = S.SeqSetDesc(1 << 33, 1, 0, 1, 1)   # non-NULL arrays that point nowhere: the size check comes first
    assert lib.seqalign_sw_stats_cross(fake, C.byref(huge), C.byref(huge), C.byref(sc), *out) == S.E_ARG
    assert "overflow" in lib.seqalign_last_error().decode()


def long_batch(len_a, len_b):
    """Three pairs; the SECOND holds sequences of len_a and len_b letters."""
    return W.from_pairs([(b"ACGT", b"ACG"), (b"A" * len_a, b"C" * len_b), (b"AC", b"AC")])


def test_length_limit_of_the_batch_calls_comes_with_the_argument_checks():
    """65 535 letters pass the check and reach the refusal of the NULL context; 65 536 in seq_a, and then in seq_b, of the second
    pair is SEQALIGN_E_TOO_LARGE with the pair named -- with a context that is never dereferenced, so before any device work."""
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    out = [S._ptr(x) for x in outputs(3)]
    ms = np.zeros(1, np.float32)
    null, fake = C.c_void_p(0), C.c_void_p(1)
    ctxs, no_ctxs = (C.c_void_p * 1)(fake.value), (C.c_void_p * 1)(0)

    def calls(d, ctx, ctx_list):
        return [("batch", lib.seqalign_sw_stats_batch(ctx, C.byref(d), C.byref(sc), *out)),
                ("multi", lib.seqalign_sw_stats_batch_multi(ctx_list, C.c_int(1), C.byref(d), C.byref(sc), *out)),
                ("time", lib.seqalign_sw_stats_time_ms(ctx, C.byref(d), C.byref(sc), C.c_int(1), S._ptr(ms)))]

    for la, lb in ((MAX_LEN, 3), (3, MAX_LEN), (MAX_LEN, MAX_LEN)):
        b = long_batch(la, lb)
        for name, rc in calls(S.batch_desc(b), null, no_ctxs):
            assert rc == S.E_ARG, (name, la, lb, rc)
    for la, lb, which in ((MAX_LEN + 1, 3, "seq_a"), (3, MAX_LEN + 1, "seq_b"), (MAX_LEN + 1, MAX_LEN + 1, "seq_a")):
        b = long_batch(la, lb)
        d = S.batch_desc(b)
        for ctx, ctx_list in ((fake, ctxs), (null, no_ctxs)):
            for name in ("batch", "multi", "time"):
                rc = dict(calls(d, ctx, ctx_list))[name]
                msg = lib.seqalign_last_error().decode()
                assert rc == S.E_TOO_LARGE, (name, la, lb, rc)
                assert "pair 1:" in msg and which in msg and "65536" in msg and "65535" in msg, (name, msg)


def test_length_limit_of_the_cross_call():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    short = W.seqset_from([b"ACGT", b"AC", b"", b"ACG"])
    null, fake = C.c_void_p(0), C.c_void_p(1)
    out = [S._ptr(x) for x in outputs(16)]
    at_limit = W.seqset_from([b"ACGT", b"A" * MAX_LEN, b"", b"ACG"])
    for q, t in ((at_limit, short), (short, at_limit)):
        dq, dt = S.seqset_desc(q), S.seqset_desc(t)
        assert lib.seqalign_sw_stats_cross(null, C.byref(dq), C.byref(dt), C.byref(sc), *out) == S.E_ARG
    over = W.seqset_from([b"ACGT", b"AC", b"A" * (MAX_LEN + 1), b"ACG"])
    for q, t, what in ((over, short, "query 2:"), (short, over, "target 2:"), (over, over, "query 2:")):
        dq, dt = S.seqset_desc(q), S.seqset_desc(t)
        for ctx in (fake, null):
            assert lib.seqalign_sw_stats_cross(ctx, C.byref(dq), C.byref(dt), C.byref(sc), *out) == S.E_TOO_LARGE, what
            msg = lib.seqalign_last_error().decode()
            assert what in msg and "65536" in msg, msg


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["sw_stats", "sw_stats_time_ms"])
def test_batch_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    good = W.from_pairs([(b"ACGT", b"ACG"), (b"", b"T")])
    fn = getattr(ctx, call)
    with pytest.raises(S.SeqAlignError) as e:
        fn(good, sc)                                   # a valid batch reaches the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_sw_stats" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        fn(long_batch(MAX_LEN, MAX_LEN), sc)           # at the limit: the same
    assert e.value.code == S.E_ARG and "seqalign_sw_stats" in str(e.value)
    for la, lb, which in ((MAX_LEN + 1, 3, "seq_a"), (3, MAX_LEN + 1, "seq_b")):
        with pytest.raises(S.SeqAlignError) as e:
            fn(long_batch(la, lb), sc)
        assert e.value.code == S.E_TOO_LARGE and "pair 1:" in str(e.value) and which in str(e.value), str(e.value)
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
    if call == "sw_stats_time_ms":
        with pytest.raises(S.SeqAlignError) as e:
            fn(good, sc, repeats=0)
        assert e.value.code == S.E_ARG and "repeats" in str(e.value)


def test_cross_wrapper_checks_its_arguments():
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    q, t = W.seqset_from([b"ACGT", b"AC"]), W.seqset_from([b"ACG", b"", b"T"])
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_stats_cross(q, t, sc)                   # valid sets reach the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_sw_stats_cross" in str(e.value)
    over = W.seqset_from([b"AC", b"A" * (MAX_LEN + 1)])
    for qq, tt, what in ((over, t, "query 1:"), (q, over, "target 1:")):
        with pytest.raises(S.SeqAlignError) as e:
            ctx.sw_stats_cross(qq, tt, sc)
        assert e.value.code == S.E_TOO_LARGE and what in str(e.value), str(e.value)
    with pytest.raises(S.SeqAlignError):
        ctx.sw_stats_cross(q, t, {"preset": "default"})
    for wrong in (W.SeqSet(q.arena, q.off.astype(np.int64), q.len), W.SeqSet(q.arena, q.off[:1], q.len), object()):
        with pytest.raises(S.SeqAlignError) as e:
            ctx.sw_stats_cross(wrong, t, sc)
        assert e.value.code == S.E_ARG
        with pytest.raises(S.SeqAlignError):
            ctx.sw_stats_cross(q, wrong, sc)
