"""CPU tier: the banded NW statistics call's surface -- exported and declared symbols, the unchanged kernel kind tables, the
argument checks of the C calls in seqalign_nw_score_banded's order (NULL arguments and repeats, then the unreadable batch, then
the width under the span call's cap; no limit on the lengths) and of the Python wrappers, all before any device is looked for:
the context handed in is never dereferenced."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

CALLS = ["seqalign_nw_stats_banded", "seqalign_nw_stats_band_time_ms"]
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"


def test_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(CALLS) <= defined, set(CALLS) - defined
    assert set(CALLS) <= set(S.EXPORTED_SYMBOLS)
    assert callable(S.Context.nw_stats_banded) and callable(S.Context.nw_stats_band_time_ms)
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in CALLS:
        assert re.search(r"^int " + name + r"\(", text, flags=re.M), name
    # the call re-uses the span call's cap: no constant of its own
    assert re.search(r"#define\s+SEQALIGN_SPAN_BAND_MAX_WIDTH\s+512\b", text)
    assert not re.search(r"#define\s+SEQALIGN_\w*STATS_BAND\w*", text)


def test_kind_tables_are_unchanged():
    """The call adds no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def _args(pairs, band):
    b = W.from_pairs(pairs)
    n = b.n_pairs
    return dict(b=b, d=S.batch_desc(b), sc=S.make_scoring({"preset": "default"}), band=np.asarray(band, np.uint32),
                os=np.zeros(n, np.int32), u=[np.zeros(n, np.uint32) for _ in range(2)], t=np.zeros(4, np.float32))


def _stats_args(k, ctx):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["band"]), P(k["os"]), *[P(x) for x in k["u"]]]


def _time_args(k, ctx, repeats=4):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["band"]), C.c_int(repeats), P(k["t"])]


def test_c_calls_refuse_null_arguments_without_a_device():
    lib = S.lib()
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")], [1, 0])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args = _stats_args(k, fake)
    assert len(args) == 7
    for i in range(len(args)):
        bad = list(args)
        bad[i] = null
        assert lib.seqalign_nw_stats_banded(*bad) == S.E_ARG, i
    args = _time_args(k, fake)
    assert len(args) == 6
    for i in (0, 1, 2, 3, 5):
        bad = list(args)
        bad[i] = null
        assert lib.seqalign_nw_stats_band_time_ms(*bad) == S.E_ARG, i
    for repeats in (0, -3):
        assert lib.seqalign_nw_stats_band_time_ms(*_time_args(k, fake, repeats)) == S.E_ARG, repeats
    # an unreadable batch: no off_a
    b = k["b"]
    bad = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert lib.seqalign_nw_stats_banded(fake, C.byref(bad), *_stats_args(k, fake)[2:]) == S.E_ARG
    assert lib.seqalign_nw_stats_band_time_ms(fake, C.byref(bad), *_time_args(k, fake)[2:]) == S.E_ARG


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


def _both_calls(lib, k, d, ctx):
    """The two calls' codes on batch `d` with k's bands, each with the last error it left."""
    out = []
    for fn, args in ((lib.seqalign_nw_stats_banded, _stats_args(k, ctx)), (lib.seqalign_nw_stats_band_time_ms, _time_args(k, ctx))):
        args[1] = C.byref(d)
        out.append((fn(*args), lib.seqalign_last_error().decode()))
    return out


def test_a_width_of_512_passes_and_513_is_refused_without_a_device():
    """Pair 0: 5 000 x 4 999 at w = 255 is 1 + 1 + 510 = 512 diagonals and passes; pair 1's w = 256 on equal lengths is 513 and
    is refused with pair and both numbers named.  With every width at 512 or below the calls pass all checks made from the
    arguments alone and reach the context, which is NULL here: E_ARG, not E_TOO_LARGE."""
    lib, fake, null = S.lib(), C.c_void_p(1), C.c_void_p(0)
    keep, d = _lengths_only([5000, 5000], [4999, 5000])
    k = _args([(b"A", b"A")] * 2, [255, 256])
    for rc, msg in _both_calls(lib, k, d, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "513" in msg and "512" in msg, (rc, msg)
    k = _args([(b"A", b"A")] * 2, [255, 2 ** 32 - 1])       # the message names the span cap, not the score call's 1 024
    for rc, msg in _both_calls(lib, k, d, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "10001" in msg and "512" in msg, (rc, msg)
    k = _args([(b"A", b"A")] * 2, [255, 255])               # 512 and 511 diagonals
    for rc, msg in _both_calls(lib, k, d, null):
        assert rc == S.E_ARG, (rc, msg)
    keep2, d2 = _lengths_only([250], [261])                 # the whole matrix of a small pair: 250 + 261 + 1 = 512
    k = _args([(b"A", b"A")], [2 ** 32 - 1])
    for rc, msg in _both_calls(lib, k, d2, null):
        assert rc == S.E_ARG, (rc, msg)
    del keep, keep2


def test_there_is_no_length_limit():
    """A 70 000-letter pair at w = 3 passes every check made from the arguments alone (seqalign_sw_stats_banded refuses it);
    len_a + len_b >= 2^31 is refused as in seqalign_nw_score_banded."""
    lib, fake, null = S.lib(), C.c_void_p(1), C.c_void_p(0)
    keep, d = _lengths_only([70000, 9], [70000, 70000])
    k = _args([(b"A", b"A")] * 2, [3, 3])
    for rc, msg in _both_calls(lib, k, d, null):
        assert rc == S.E_ARG, (rc, msg)                     # the NULL context is what is refused
    keep2, d2 = _lengths_only([5, 2 ** 30], [5, 2 ** 30])
    for rc, msg in _both_calls(lib, k, d2, fake):
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "2^31" in msg, (rc, msg)
    del keep, keep2


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_stats_banded", "nw_stats_band_time_ms"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    fn = getattr(ctx, call)
    for band in (3, [3, 0], 2 ** 32 - 1, np.array([5, 7], np.int64)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, band)                                 # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and "seqalign_nw_stats_band" in str(e.value)
    for band in ([1, 2, 3], 1.5, "3", None, 2 ** 32, -1, [[1, 2]]):   # wrong dtypes, shapes and ranges
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, band)
        assert e.value.code == S.E_ARG and "band:" in str(e.value), band
    with pytest.raises(S.SeqAlignError) as e:
        fn(b, {"preset": "default"}, 1)                     # not a scoring_t
    assert e.value.code == S.E_ARG
    outside = W.Batch(b.arena, b.off_a.copy(), b.len_a.copy(), b.off_b.copy(), b.len_b.copy())
    outside.off_b[0] = np.uint64(b.arena.nbytes)
    with pytest.raises(S.SeqAlignError) as e:
        fn(outside, sc, 1)                                  # a sequence past the arena's end
    assert e.value.code == S.E_ARG and "outside" in str(e.value)
    if call == "nw_stats_band_time_ms":
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, 1, repeats=0)
        assert e.value.code == S.E_ARG and "repeats" in str(e.value)
