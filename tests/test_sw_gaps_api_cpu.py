"""CPU tier: the surface of the SW gap-run calls (seqalign_sw_gaps_batch / _banded / _banded_wide and the two timing
hooks) -- exported and declared symbols, the wrappers, the unchanged kernel kind tables, and the argument checks of the C calls
in the span calls' order, all before any device is looked for: the context handed in is never dereferenced.  There is no
length limit: a sequence of 65 536 letters, which every sw_stats call refuses, passes every check of all three calls."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

BATCH, NARROW, WIDE = "seqalign_sw_gaps_batch", "seqalign_sw_gaps_banded", "seqalign_sw_gaps_banded_wide"
TIME, BAND_TIME = "seqalign_sw_gaps_time_ms", "seqalign_sw_gaps_band_time_ms"
SYMBOLS = [BATCH, NARROW, WIDE, TIME, BAND_TIME]
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _decl(text, name):
    m = re.search(r"^int " + name + r"\((.*?)\);", text, flags=re.M | re.S)
    assert m, name
    return [re.sub(r"\bout_\w+", "out", w) for w in m.group(1).split()]     # the argument list without the outputs' names


def test_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)
    assert len(S.EXPORTED_SYMBOLS) == len(set(S.EXPORTED_SYMBOLS))
    for f in ("sw_gaps", "sw_gaps_banded", "sw_gaps_banded_wide", "sw_gaps_time_ms", "sw_gaps_band_time_ms"):
        assert callable(getattr(S.Context, f)), f
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    # five results: the argument lists are the span calls', word for word but for the outputs' names
    assert _decl(text, BATCH) == _decl(text, "seqalign_sw_span_batch")
    assert _decl(text, NARROW) == _decl(text, "seqalign_sw_span_banded") == _decl(text, WIDE)
    assert _decl(text, TIME) == _decl(text, "seqalign_sw_stats_time_ms")
    assert _decl(text, BAND_TIME) == _decl(text, "seqalign_sw_stats_band_time_ms")
    # ... and the counts calls', whose checks, bytes and chunks these calls share
    for name in SYMBOLS:
        assert _decl(text, name) == _decl(text, name.replace("sw_gaps", "sw_counts")), name
    raw = HEADER.read_text()
    for out in ("out_gap_runs_a", "out_gap_runs_b"):
        assert raw.count(out) >= 3, out
    assert not re.search(r"#define\s+SEQALIGN_\w*GAPS\w*", text)                    # no constant of their own
    assert re.search(r"^#define SEQALIGN_SW_STATS_MAX_LEN 65535u$", HEADER.read_text(), re.M)   # sw_stats keeps its limit


def test_kind_tables_are_unchanged():
    """The calls add no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
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
                ms=np.zeros(1, np.float32))


def _call_args(name, k, ctx, d=None):
    P = S._ptr
    head = [ctx, C.byref(d if d is not None else k["d"]), C.byref(k["sc"])]
    band = [P(k["lo"]), P(k["hi"])]
    outs = [P(k["os"]), *[P(x) for x in k["u"]]]
    return {BATCH: head + outs, NARROW: head + band + outs, WIDE: head + band + outs,
            TIME: head + [C.c_int(1), P(k["ms"])],
            BAND_TIME: head + band + [C.c_int(1), P(k["ms"])]}[name.replace("sw_span", "sw_gaps").replace("sw_counts", "sw_gaps")]   # (the span and counts siblings: same lists)


def _call(lib, name, k, ctx, d=None):
    return getattr(lib, name)(*_call_args(name, k, ctx, d)), lib.seqalign_last_error().decode()


@pytest.mark.parametrize("name", SYMBOLS)
def test_c_calls_refuse_null_and_bad_arguments_without_a_device(name):
    lib = S.lib()
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")], [-1, 0], [1, 0])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args = _call_args(name, k, fake)
    assert len(args) == {BATCH: 8, NARROW: 10, WIDE: 10, TIME: 5, BAND_TIME: 7}[name]
    for i, arg in enumerate(args):
        if isinstance(arg, C.c_int):
            continue
        bad = list(args)
        bad[i] = null
        assert getattr(lib, name)(*bad) == S.E_ARG, i
    if name in (TIME, BAND_TIME):                  # repeats <= 0; an empty batch
        bad = list(args)
        bad[-2] = C.c_int(0)
        assert getattr(lib, name)(*bad) == S.E_ARG
    b = k["b"]
    unreadable = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    if name in (NARROW, WIDE, BAND_TIME):          # the band calls read the batch before the context: the span calls' order
        assert _call(lib, name, k, fake, unreadable)[0] == S.E_ARG
        k2 = _args([(b"ACGT", b"ACG"), (b"AC", b"T")], [-1, 2], [1, 1])
        rc, msg = _call(lib, name, k2, fake)
        assert rc == S.E_ARG and msg.startswith("pair 1:") and "diag_lo" in msg, (rc, msg)
        assert (rc, msg) == _call(lib, name.replace("sw_gaps", "sw_span"), k2, fake)      # the span call's status and message
        assert (rc, msg) == _call(lib, name.replace("sw_gaps", "sw_counts"), k2, fake)    # and the counts call's
    else:                                          # seqalign_sw_span_batch's order: the context first
        assert _call(lib, name, k, null, unreadable)[0] == S.E_ARG


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


@pytest.mark.parametrize("lo, hi, width", [(-256, 256, 513), (-512, 512, 1025), (INT32_MIN, INT32_MAX, 10001)])
def test_width_513_is_too_large_for_the_narrow_call_only(lo, hi, width):
    lib, fake, null = S.lib(), C.c_void_p(1), C.c_void_p(0)
    keep, d = _lengths_only([5000, 5000], [4999, 5000])
    k = _args([(b"A", b"A")] * 2, [-255, lo], [255, hi])
    for name in (NARROW, BAND_TIME):
        rc, msg = _call(lib, name, k, fake, d)
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and str(width) in msg, (name, rc, msg)
    assert _call(lib, NARROW, k, fake, d) == _call(lib, "seqalign_sw_span_banded", k, fake, d)     # the span call's message
    rc, msg = _call(lib, WIDE, k, null, d)         # every check passed: the NULL context is what is refused
    assert rc == S.E_ARG, (rc, msg)
    k512 = _args([(b"A", b"A")] * 2, [-255, -256], [255, 255])
    assert _call(lib, NARROW, k512, null, d)[0] == S.E_ARG      # 512 diagonals: legal
    del keep


def test_the_wide_call_keeps_the_span_calls_length_rule():
    lib, fake = S.lib(), C.c_void_p(1)
    keep, d = _lengths_only([5, 2 ** 30], [5, 2 ** 30])
    k = _args([(b"A", b"A")] * 2, [-3, INT32_MIN], [3, INT32_MAX])
    for name in (WIDE, NARROW):
        rc, msg = _call(lib, name, k, fake, d)
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "2^31" in msg, (name, rc, msg)
    del keep


def test_65536_letters_pass_every_check_of_all_three_calls():
    """What seqalign_sw_stats_* refuses from the descriptors alone is no error here.  The checks that CAN fail still run over
    such a batch (a later pair's band is refused, pair named, with a context that is never dereferenced), and with nothing to
    refuse the call goes on to the context, NULL here: E_ARG, not E_TOO_LARGE."""
    lib, fake, null = S.lib(), C.c_void_p(1), C.c_void_p(0)
    keep, d = _lengths_only([65536, 5, 70000], [5, 65536, 200000])
    ok = _args([(b"A", b"A")] * 3, [-3, -3, -3], [3, 3, 3])
    for stats in ("seqalign_sw_stats_banded", "seqalign_sw_stats_banded_wide"):
        rc, msg = _call(lib, stats.replace("sw_stats", "sw_gaps"), ok, null, d)
        assert rc == S.E_ARG, (stats, rc, msg)
        P = S._ptr
        six = [np.zeros(3, np.uint32) for _ in range(6)]
        rc = getattr(lib, stats)(fake, C.byref(d), C.byref(ok["sc"]), P(ok["lo"]), P(ok["hi"]), P(ok["os"]), *[P(x) for x in six])
        assert rc == S.E_TOO_LARGE and "65536" in lib.seqalign_last_error().decode()      # the sibling refuses the same batch
    for name in (BATCH, TIME, BAND_TIME):
        rc, msg = _call(lib, name, ok, null, d)
        assert rc == S.E_ARG, (name, rc, msg)
    bad_band = _args([(b"A", b"A")] * 3, [-3, -3, 4], [3, 3, 3])
    for name in (NARROW, WIDE, BAND_TIME):
        rc, msg = _call(lib, name, bad_band, fake, d)
        assert rc == S.E_ARG and msg.startswith("pair 2:") and "diag_lo" in msg, (name, rc, msg)
    too_wide = _args([(b"A", b"A")] * 3, [-3, -3, -256], [3, 3, 256])
    rc, msg = _call(lib, NARROW, too_wide, fake, d)
    assert rc == S.E_TOO_LARGE and msg.startswith("pair 2:") and "513" in msg and "letters" not in msg, (rc, msg)
    del keep


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


def test_python_wrappers_check_their_arguments():
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    long_b = W.from_pairs([(b"A" * 65536, b"C" * 3), (b"AC", b"C" * 65536)])
    for fn, sym in ((ctx.sw_gaps, BATCH), (ctx.sw_gaps_time_ms, TIME)):
        for batch in (b, long_b):                             # no length limit in the wrapper either
            with pytest.raises(S.SeqAlignError) as e:
                fn(batch, sc)
            assert e.value.code == S.E_ARG and sym in str(e.value)
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, {"preset": "default"})
        assert e.value.code == S.E_ARG
        with pytest.raises(S.SeqAlignError):
            fn(object(), sc)
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_gaps_time_ms(b, sc, repeats=0)
    assert e.value.code == S.E_ARG and "repeats" in str(e.value)
    for fn, sym in ((ctx.sw_gaps_banded, NARROW), (ctx.sw_gaps_banded_wide, WIDE), (ctx.sw_gaps_band_time_ms, BAND_TIME)):
        for batch, lo, hi in ((b, -3, 3), (b, [-3, 0], [3, 0]), (long_b, -100, 100), (b, np.array([5, -7], np.int64), 9)):
            with pytest.raises(S.SeqAlignError) as e:
                fn(batch, sc, lo, hi)                         # valid arguments reach the C call, which refuses the NULL context
            assert e.value.code == S.E_ARG and sym in str(e.value)
        for lo in ([1, 2, 3], 1.5, "3", None, 2 ** 31, [[1, 2]]):
            with pytest.raises(S.SeqAlignError) as e:
                fn(b, sc, lo, 2 ** 31 - 1)
            assert e.value.code == S.E_ARG and "diag_lo:" in str(e.value), lo
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, {"preset": "default"}, -1, 1)
        assert e.value.code == S.E_ARG
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_gaps_band_time_ms(b, sc, -1, 1, repeats=0)
    assert e.value.code == S.E_ARG and "repeats" in str(e.value)
