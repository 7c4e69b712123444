"""CPU tier: the banded SW hit-span call's surface -- exported and declared symbols, the unchanged kernel kind tables, the
argument checks of the C calls (E_ARG, E_TOO_LARGE with the span call's own cap) and of the Python wrappers, all before any
device is looked for: the context handed in is never dereferenced."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

CALLS = ["seqalign_sw_span_banded", "seqalign_sw_span_band_time_ms"]
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def test_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(CALLS) <= defined, set(CALLS) - defined
    assert set(CALLS) <= set(S.EXPORTED_SYMBOLS)
    assert callable(S.Context.sw_span_banded) and callable(S.Context.sw_span_band_time_ms)
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+SEQALIGN_SPAN_BAND_MAX_WIDTH\s+512\b", text)


def test_kind_tables_are_unchanged():
    """The call adds no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def _args(pairs, lo, hi):
    b = W.from_pairs(pairs)
    n = b.n_pairs
    return dict(b=b, d=S.batch_desc(b), sc=S.make_scoring({"preset": "default"}), lo=np.asarray(lo, np.int32),
                hi=np.asarray(hi, np.int32), os=np.zeros(n, np.int32), u=[np.zeros(n, np.uint32) for _ in range(4)],
                t=np.zeros(4, np.float32))


def _span_args(k, ctx):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["lo"]), P(k["hi"]), P(k["os"]), *[P(x) for x in k["u"]]]


def _time_args(k, ctx, repeats=4):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["lo"]), P(k["hi"]), C.c_int(repeats), P(k["t"])]


def test_c_calls_refuse_null_arguments_without_a_device():
    lib = S.lib()
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")], [-1, 0], [1, 0])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args = _span_args(k, fake)
    for i in range(len(args)):
        bad = list(args)
        bad[i] = null
        assert lib.seqalign_sw_span_banded(*bad) == S.E_ARG, i
    args = _time_args(k, fake)
    for i in (0, 1, 2, 3, 4, 6):
        bad = list(args)
        bad[i] = null
        assert lib.seqalign_sw_span_band_time_ms(*bad) == S.E_ARG, i
    for repeats in (0, -3):
        assert lib.seqalign_sw_span_band_time_ms(*_time_args(k, fake, repeats)) == S.E_ARG, repeats
    # an unreadable batch: no off_a
    b = k["b"]
    bad = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert lib.seqalign_sw_span_banded(fake, C.byref(bad), *_span_args(k, fake)[2:]) == S.E_ARG
    assert lib.seqalign_sw_span_band_time_ms(fake, C.byref(bad), *_time_args(k, fake)[2:]) == S.E_ARG


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


def _both_calls(lib, k, d, fake):
    """The two calls' codes on batch `d` with k's bounds, each with the last error it left."""
    out = []
    for fn, args in ((lib.seqalign_sw_span_banded, _span_args(k, fake)), (lib.seqalign_sw_span_band_time_ms, _time_args(k, fake))):
        args[1] = C.byref(d)
        out.append((fn(*args), lib.seqalign_last_error().decode()))
    return out


def test_c_calls_refuse_crossed_bounds_without_a_device():
    """diag_lo > diag_hi as given is the caller's mistake, whatever clipping would make of it: E_ARG, the pair named."""
    lib, fake = S.lib(), C.c_void_p(1)
    keep, d = _lengths_only([100, 100, 100], [90, 90, 90])
    k = _args([(b"A", b"A")] * 3, [-5, 4, 200], [5, 3, 150])
    for rc, msg in _both_calls(lib, k, d, fake):
        assert rc == S.E_ARG and msg.startswith("pair 1:"), (rc, msg)
    del keep


def test_c_calls_refuse_a_band_of_513_diagonals_without_a_device():
    """Found from the lengths and the bounds alone: the sequences are not read, no device is looked for, pair and width are
    named.  Pair 0: bounds INT32_MIN / INT32_MAX on a 250 x 261 pair clip to 261 + 250 + 1 = 512 diagonals and pass the check --
    the calls go on to pair 1, whose 513 they refuse."""
    lib, fake = S.lib(), C.c_void_p(1)
    keep, d = _lengths_only([250, 5000], [261, 5000])
    k = _args([(b"A", b"A")] * 2, [INT32_MIN, -256], [INT32_MAX, 256])
    for rc, msg in _both_calls(lib, k, d, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "513" in msg and "512" in msg, (rc, msg)
    # bounds wholly right of the main diagonal: pair 0's clip to 201 diagonals, pair 1's are 513 as they stand
    k = _args([(b"A", b"A")] * 2, [50, 7], [1123, 519])
    for rc, msg in _both_calls(lib, k, d, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "513" in msg, (rc, msg)
    # the message names the span call's cap, not the score call's 1 024
    k = _args([(b"A", b"A")] * 2, [0, -512], [0, 512])
    for rc, msg in _both_calls(lib, k, d, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "1025" in msg and "512" in msg, (rc, msg)
    # clipping comes first: 2 000 diagonals as given, 251 inside the matrix; then a pair that is too long
    keep2, d2 = _lengths_only([250, 2 ** 30], [261, 2 ** 30])
    k = _args([(b"A", b"A")] * 2, [0, 0], [1999, 0])
    for rc, msg in _both_calls(lib, k, d2, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "2^31" in msg, (rc, msg)
    del keep, keep2


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["sw_span_banded", "sw_span_band_time_ms"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    fn = getattr(ctx, call)
    for lo, hi in ((-3, 3), ([-3, 0], [3, 0]), (INT32_MIN, INT32_MAX), (np.array([5, -7], np.int64), 9)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, lo, hi)                             # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and "seqalign_sw_span_band" in str(e.value)
    for lo in ([1, 2, 3], 1.5, "3", None, 2 ** 31, -2 ** 31 - 1, [[1, 2]]):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, lo, 2 ** 31 - 1)
        assert e.value.code == S.E_ARG and "diag_lo:" in str(e.value), lo
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, -5, lo)
        assert e.value.code == S.E_ARG and "diag_hi:" in str(e.value), lo
    with pytest.raises(S.SeqAlignError) as e:
        fn(b, {"preset": "default"}, -1, 1)               # not a scoring_t
    assert e.value.code == S.E_ARG
    outside = W.Batch(b.arena, b.off_a.copy(), b.len_a.copy(), b.off_b.copy(), b.len_b.copy())
    outside.off_b[0] = np.uint64(b.arena.nbytes)
    with pytest.raises(S.SeqAlignError) as e:
        fn(outside, sc, -1, 1)                            # a sequence past the arena's end
    assert e.value.code == S.E_ARG and "outside" in str(e.value)
    if call == "sw_span_band_time_ms":
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, -1, 1, repeats=0)
        assert e.value.code == S.E_ARG and "repeats" in str(e.value)
