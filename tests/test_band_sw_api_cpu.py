"""CPU tier: the banded SW calls' surface -- exported and declared symbols, the argument checks of the C calls (E_ARG,
E_TOO_LARGE) and of the Python wrappers, all before any device is looked for: the context handed in is never dereferenced."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

CALLS = ["seqalign_sw_score_banded", "seqalign_sw_align_banded", "seqalign_sw_band_score_time_ms"]
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def test_band_sw_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(CALLS) <= defined, set(CALLS) - defined
    assert set(CALLS) <= set(S.EXPORTED_SYMBOLS)
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    # the second launch record got no new kind
    lib = S.lib()
    assert [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(5)] == [b"band_score", b"band_fill", b"band_walk", None, None]


def _args(pairs, lo, hi):
    b = W.from_pairs(pairs)
    n = b.n_pairs
    return dict(b=b, d=S.batch_desc(b), sc=S.make_scoring({"preset": "default"}), lo=np.asarray(lo, np.int32),
                hi=np.asarray(hi, np.int32), ms=np.ones(n, np.int32), hits=(S.SwHit * n)(), nh=C.c_uint64(7),
                oa=np.zeros(4096, np.uint8), ob=np.zeros(4096, np.uint8), os=np.zeros(n, np.int32),
                ea=np.zeros(n, np.uint32), eb=np.zeros(n, np.uint32), t=np.zeros(4, np.float32))


def _score_args(k, ctx):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["lo"]), P(k["hi"]), P(k["os"]), P(k["ea"]), P(k["eb"])]


def _align_args(k, ctx):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["lo"]), P(k["hi"]), P(k["ms"]), k["hits"], C.c_uint64(len(k["hits"])),
            C.byref(k["nh"]), P(k["oa"]), P(k["ob"]), C.c_uint64(4096)]


def _time_args(k, ctx, repeats=4):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["lo"]), P(k["hi"]), C.c_int(repeats), P(k["t"])]


def test_c_calls_refuse_null_arguments_without_a_device():
    lib = S.lib()
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")], [-1, 0], [1, 0])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args = _score_args(k, fake)
    for i in range(len(args)):
        bad = list(args)
        bad[i] = null
        assert lib.seqalign_sw_score_banded(*bad) == S.E_ARG, i
    args = _align_args(k, fake)
    for i in (0, 1, 2, 3, 4, 5, 6, 8, 9, 10):      # 7 and 11 are the capacities
        bad = list(args)
        bad[i] = null
        assert lib.seqalign_sw_align_banded(*bad) == S.E_ARG, i
    args = _time_args(k, fake)
    for i in (0, 1, 2, 3, 4, 6):
        bad = list(args)
        bad[i] = null
        assert lib.seqalign_sw_band_score_time_ms(*bad) == S.E_ARG, i
    for repeats in (0, -3):
        assert lib.seqalign_sw_band_score_time_ms(*_time_args(k, fake, repeats)) == S.E_ARG, repeats
    # an unreadable batch: no off_a
    b = k["b"]
    bad = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert lib.seqalign_sw_score_banded(fake, C.byref(bad), *_score_args(k, fake)[2:]) == S.E_ARG
    assert lib.seqalign_sw_align_banded(fake, C.byref(bad), *_align_args(k, fake)[2:]) == S.E_ARG
    assert lib.seqalign_sw_band_score_time_ms(fake, C.byref(bad), *_time_args(k, fake)[2:]) == S.E_ARG


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


def _three_calls(lib, k, d, fake):
    """The three calls' codes on batch `d` with k's bounds, each with the last error it left."""
    out = []
    for fn, args in ((lib.seqalign_sw_score_banded, _score_args(k, fake)), (lib.seqalign_sw_align_banded, _align_args(k, fake)),
                     (lib.seqalign_sw_band_score_time_ms, _time_args(k, fake))):
        args[1] = C.byref(d)
        out.append((fn(*args), lib.seqalign_last_error().decode()))
    return out


def test_c_calls_refuse_crossed_bounds_without_a_device():
    """diag_lo > diag_hi as given is the caller's mistake, whatever clipping would make of it: E_ARG, the pair named."""
    lib, fake = S.lib(), C.c_void_p(1)
    keep, d = _lengths_only([100, 100, 100], [90, 90, 90])
    k = _args([(b"A", b"A")] * 3, [-5, 4, 200], [5, 3, 150])
    for rc, msg in _three_calls(lib, k, d, fake):
        assert rc == S.E_ARG and msg.startswith("pair 1:"), (rc, msg)
    assert k["nh"].value == 0                      # the align call zeroes *n_hits before it looks at anything
    del keep


def test_c_calls_refuse_a_band_of_1025_diagonals_without_a_device():
    """Found from the lengths and the bounds alone: the sequences are not read, no device is looked for, pair and width are
    named.  Pair 0: bounds INT32_MIN / INT32_MAX on a 500 x 523 pair clip to 523 + 500 + 1 = 1 024 diagonals and are
    accepted -- the calls go on to pair 1, whose 1 025 they refuse."""
    lib, fake = S.lib(), C.c_void_p(1)
    keep, d = _lengths_only([500, 5000], [523, 5000])
    k = _args([(b"A", b"A")] * 2, [INT32_MIN, -512], [INT32_MAX, 512])
    for rc, msg in _three_calls(lib, k, d, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "1025" in msg, (rc, msg)
    # bounds wholly right of the main diagonal: pair 0's clip to 401 diagonals, pair 1's are 1 025 as they stand
    k = _args([(b"A", b"A")] * 2, [100, 7], [1123, 1031])
    for rc, msg in _three_calls(lib, k, d, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "1025" in msg, (rc, msg)
    # clipping comes first: 2 000 diagonals as given, 501 inside the matrix; then a pair that is too long
    keep2, d2 = _lengths_only([500, 2 ** 30], [523, 2 ** 30])
    k = _args([(b"A", b"A")] * 2, [0, 0], [1999, 0])
    for rc, msg in _three_calls(lib, k, d2, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "2^31" in msg, (rc, msg)
    del keep, keep2


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["sw_score_banded", "sw_align_banded", "sw_band_score_time_ms"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    tail = (1,) if call == "sw_align_banded" else ()
    fn = getattr(ctx, call)
    for lo, hi in ((-3, 3), ([-3, 0], [3, 0]), (INT32_MIN, INT32_MAX), (np.array([5, -7], np.int64), 9)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, lo, hi, *tail)                      # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and "seqalign_sw_" in str(e.value)
    for lo in ([1, 2, 3], 1.5, "3", None, 2 ** 31, -2 ** 31 - 1, [[1, 2]]):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, lo, 2 ** 31 - 1, *tail)
        assert e.value.code == S.E_ARG and "diag_lo:" in str(e.value), lo
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, -5, lo, *tail)
        assert e.value.code == S.E_ARG and "diag_hi:" in str(e.value), lo
    with pytest.raises(S.SeqAlignError) as e:
        fn(b, {"preset": "default"}, -1, 1, *tail)        # not a scoring_t
    assert e.value.code == S.E_ARG
    if call == "sw_align_banded":
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, -1, 1, [1, 2, 3])
        assert e.value.code == S.E_ARG and "min_score" in str(e.value)
