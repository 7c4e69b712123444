"""CPU tier: the wide banded SW hit-span call's surface -- the exported and declared symbol, the wrapper, the unchanged kernel
kind tables, and the argument checks of the C call: seqalign_sw_span_banded's checks in their order with the width check left
out (NULL arguments, then per pair the unreadable batch, diag_lo > diag_hi and len_a + len_b >= 2^31) and no limit on the
lengths, all before any device is looked for: the context handed in is never dereferenced.  Modelled on
test_sw_stats_banded_wide_api_cpu.py."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

CALL = "seqalign_sw_span_banded_wide"
NARROW = "seqalign_sw_span_banded"
STATS_WIDE = "seqalign_sw_stats_banded_wide"
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def test_symbol_is_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert CALL in defined and CALL in S.EXPORTED_SYMBOLS
    assert callable(S.Context.sw_span_banded_wide)
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decl = re.search(r"^int " + CALL + r"\((.*?)\);", text, flags=re.M | re.S)
    narrow = re.search(r"^int " + NARROW + r"\((.*?)\);", text, flags=re.M | re.S)
    assert decl and narrow and decl.group(1).split() == narrow.group(1).split()      # the narrow call's argument list, word for word
    assert not re.search(r"#define\s+SEQALIGN_\w*WIDE\w*", text)                      # no constant of its own
    assert re.findall(r"#define\s+(SEQALIGN_\w*SPAN_BAND\w*)", text) == ["SEQALIGN_SPAN_BAND_MAX_WIDTH"]
    assert re.search(r"#define\s+SEQALIGN_SPAN_BAND_MAX_WIDTH\s+512\b", text)         # the narrow call's cap stays


def test_kind_tables_are_unchanged():
    """The call adds no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def _args(pairs, lo, hi, words=4):
    b = W.from_pairs(pairs)
    n = b.n_pairs
    return dict(b=b, d=S.batch_desc(b), sc=S.make_scoring({"preset": "default"}), lo=np.asarray(lo, np.int32),
                hi=np.asarray(hi, np.int32), os=np.zeros(n, np.int32), u=[np.zeros(n, np.uint32) for _ in range(words)])


def _span_args(k, ctx):
    P = S._ptr
    return [ctx, C.byref(k["d"]), C.byref(k["sc"]), P(k["lo"]), P(k["hi"]), P(k["os"]), *[P(x) for x in k["u"]]]


def test_c_call_refuses_null_arguments_without_a_device():
    lib = S.lib()
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")], [-1, 0], [1, 0])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args = _span_args(k, fake)
    assert len(args) == 10
    for i in range(len(args)):
        bad = list(args)
        bad[i] = null
        assert getattr(lib, CALL)(*bad) == S.E_ARG, i
    # an unreadable batch: no off_a
    b = k["b"]
    bad = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert getattr(lib, CALL)(fake, C.byref(bad), *_span_args(k, fake)[2:]) == S.E_ARG
    # diag_lo above diag_hi, the pair named, in the narrow call's words
    k2 = _args([(b"ACGT", b"ACG"), (b"AC", b"T")], [-1, 2], [1, 1])
    assert getattr(lib, CALL)(*_span_args(k2, fake)) == S.E_ARG
    msg = lib.seqalign_last_error().decode()
    assert msg.startswith("pair 1:") and "diag_lo" in msg, msg
    assert getattr(lib, NARROW)(*_span_args(k2, fake)) == S.E_ARG and lib.seqalign_last_error().decode() == msg


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


def _call(lib, name, k, d, ctx):
    args = _span_args(k, ctx)
    args[1] = C.byref(d)
    return getattr(lib, name)(*args), lib.seqalign_last_error().decode()


@pytest.mark.parametrize("lo, hi, width", [(-256, 256, 513), (-512, 512, 1025), (INT32_MIN, INT32_MAX, 10001)])
def test_any_width_passes_where_the_narrow_call_refuses(lo, hi, width):
    """5 000 x 5 000: the narrow call refuses the clipped band from the arguments alone, pair and width named; the wide call
    passes every such check and reaches the context, which is NULL here: E_ARG, not E_TOO_LARGE."""
    lib, fake, null = S.lib(), C.c_void_p(1), C.c_void_p(0)
    keep, d = _lengths_only([5000, 5000], [4999, 5000])
    k = _args([(b"A", b"A")] * 2, [-255, lo], [255, hi])
    rc, msg = _call(lib, NARROW, k, d, fake)
    assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and str(width) in msg, (rc, msg)
    rc, msg = _call(lib, CALL, k, d, null)
    assert rc == S.E_ARG, (rc, msg)
    del keep


def test_no_limit_on_the_lengths():
    """A pair of 70 000 letters passes every check (the NULL context is reached: E_ARG) where seqalign_sw_stats_banded_wide
    refuses it from the lengths alone; so do lengths just below the 2^31 limit on their sum."""
    lib, fake, null = S.lib(), C.c_void_p(1), C.c_void_p(0)
    k = _args([(b"A", b"A")] * 2, [-3, INT32_MIN], [3, INT32_MAX])
    k7 = _args([(b"A", b"A")] * 2, [-3, INT32_MIN], [3, INT32_MAX], words=6)
    for la, lb in (([5, 70000], [5, 180]), ([180, 5], [70000, 5]), ([70000, 70000], [70000, 70000]), ([5, 2 ** 30], [5, 2 ** 30 - 1])):
        keep, d = _lengths_only(la, lb)
        rc, msg = _call(lib, CALL, k, d, null)
        assert rc == S.E_ARG, (la, lb, rc, msg)
        rc, msg = _call(lib, STATS_WIDE, k7, d, fake)
        assert rc == S.E_TOO_LARGE and "letters" in msg, (la, lb, rc, msg)
        del keep


def test_the_per_pair_checks_keep_their_order():
    """Per pair, the lowest first: diag_lo > diag_hi (E_ARG), then len_a + len_b >= 2^31 (E_TOO_LARGE); the narrow call reports
    the same pair with the same words."""
    lib, fake = S.lib(), C.c_void_p(1)
    big, small = ([5, 2 ** 30], [5, 2 ** 30]), ([2 ** 30, 5], [2 ** 30, 5])
    keep, d = _lengths_only(*big)                               # the sum in pair 1
    k = _args([(b"A", b"A")] * 2, [-3, -3], [3, 3])
    for name in (CALL, NARROW):
        rc, msg = _call(lib, name, k, d, fake)
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and "2^31" in msg, (name, rc, msg)
    k = _args([(b"A", b"A")] * 2, [4, -3], [3, 3])              # pair 0's bounds come before pair 1's lengths
    for name in (CALL, NARROW):
        rc, msg = _call(lib, name, k, d, fake)
        assert rc == S.E_ARG and msg.startswith("pair 0:") and "diag_lo" in msg, (name, rc, msg)
    k = _args([(b"A", b"A")] * 2, [-3, 4], [3, 3])              # within pair 1 the bounds come before the lengths
    for name in (CALL, NARROW):
        rc, msg = _call(lib, name, k, d, fake)
        assert rc == S.E_ARG and msg.startswith("pair 1:") and "diag_lo" in msg, (name, rc, msg)
    keep2, d2 = _lengths_only(*small)                           # pair 0's lengths come before pair 1's bounds
    for name in (CALL, NARROW):
        rc, msg = _call(lib, name, k, d2, fake)
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 0:") and "2^31" in msg, (name, rc, msg)
    del keep, keep2


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


def test_python_wrapper_checks_its_arguments():
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    fn = ctx.sw_span_banded_wide
    for lo, hi in ((-3, 3), ([-3, 0], [3, 0]), (INT32_MIN, INT32_MAX), (np.array([5, -7], np.int64), 9)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, lo, hi)                             # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and CALL in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        ctx.sw_span_banded(b, sc, -3, 3)                  # the narrow wrapper still names its own call
    assert e.value.code == S.E_ARG and NARROW in str(e.value) and CALL not in str(e.value)
    for lo in ([1, 2, 3], 1.5, "3", None, 2 ** 31, -2 ** 31 - 1, [[1, 2]]):   # wrong dtypes, shapes and ranges
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
