"""CPU tier: the long-pair alignment calls' surface -- exported symbols, the three kernel kind names, the argument checks of the
C calls (E_ARG, E_TOO_LARGE) and of the Python wrappers, all before any device is looked for."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

SYMBOLS = ["seqalign_nw_align_long", "seqalign_sw_align_long"]


def test_long_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= defined, set(SYMBOLS) - defined
    assert set(SYMBOLS) <= set(S.EXPORTED_SYMBOLS)


def test_long_kernel_kinds_follow_score_select_and_fill_the_table():
    names = [S.lib().seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    at = names.index(b"score_select")
    assert names[at + 1:at + 4] == [b"long_forward", b"long_block", b"long_walk"]
    assert at + 4 == S.K_MAX                      # SEQALIGN_K_COUNT is exactly SEQALIGN_K_MAX
    assert names[S.K_MAX] is None


def test_long_block_rows_is_a_documented_option():
    assert S.OPTION_DEFAULTS["long_block_rows"] == 0
    header = (S.PKG_ROOT.parent / "include" / "seqalign_hip.h").read_text()
    assert "long_block_rows" in header and "seqalign_nw_align_long" in header


def _batch(pairs):
    return W.from_pairs(pairs)


def _nw(lib, ctx, d, sc, so, oa, ob, ol, os_):
    return lib.seqalign_nw_align_long(ctx, d, sc, so, oa, ob, ol, os_)


def _sw(lib, ctx, d, sc, ms, hits, cap, nh, oa, ob, scap):
    return lib.seqalign_sw_align_long(ctx, d, sc, ms, hits, C.c_uint64(cap), nh, oa, ob, C.c_uint64(scap))


def test_c_calls_refuse_null_arguments_without_a_device():
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    b = _batch([(b"ACGT", b"ACG"), (b"", b"T")])
    d = S.batch_desc(b)
    so, out_len, score = np.zeros(2, np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.int32)
    so[1] = 8
    oa, ob = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    ms = np.zeros(2, np.int32)
    hits = (S.SwHit * 4)()
    nh = C.c_uint64(7)
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    P = S._ptr
    nw_args = [fake, C.byref(d), C.byref(sc), P(so), P(oa), P(ob), P(out_len), P(score)]
    for k in range(len(nw_args)):
        args = list(nw_args)
        args[k] = null
        assert _nw(lib, *args) == S.E_ARG, k
    sw_args = [fake, C.byref(d), C.byref(sc), P(ms), hits, 4, C.byref(nh), P(oa), P(ob), 32]
    for k in (0, 1, 2, 3, 4, 6, 7, 8):
        args = list(sw_args)
        args[k] = null
        assert _sw(lib, *args) == S.E_ARG, k
    # a batch whose arrays are missing
    bad = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert _nw(lib, fake, C.byref(bad), C.byref(sc), P(so), P(oa), P(ob), P(out_len), P(score)) == S.E_ARG
    assert _sw(lib, fake, C.byref(bad), C.byref(sc), P(ms), hits, 4, C.byref(nh), P(oa), P(ob), 32) == S.E_ARG
    assert nh.value == 0                         # *n_hits is cleared before the batch is looked at


def test_c_calls_refuse_pairs_past_32_bit_lengths_without_a_device():
    """len_a + len_b >= 2^32 - 1 is SEQALIGN_E_TOO_LARGE, found from the lengths alone (the sequences are not read)."""
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    arena = np.zeros(16, np.uint8)
    off = np.zeros(1, np.uint64)
    la, lb = np.array([0xFFFFFFFF - 5], np.uint32), np.array([5], np.uint32)
    d = S.BatchDesc(1, arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data, off.ctypes.data, lb.ctypes.data)
    fake, P = C.c_void_p(1), S._ptr
    so, out_len, score = np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.int32)
    oa = np.zeros(8, np.uint8)
    assert lib.seqalign_nw_align_long(fake, C.byref(d), C.byref(sc), P(so), P(oa), P(oa), P(out_len), P(score)) == S.E_TOO_LARGE
    hits, nh, ms = (S.SwHit * 1)(), C.c_uint64(0), np.zeros(1, np.int32)
    assert lib.seqalign_sw_align_long(fake, C.byref(d), C.byref(sc), P(ms), hits, C.c_uint64(1), C.byref(nh), P(oa), P(oa),
                                      C.c_uint64(8)) == S.E_TOO_LARGE
    lb[0] = 6   # (2^32 - 1 exactly)
    assert lib.seqalign_nw_align_long(fake, C.byref(d), C.byref(sc), P(so), P(oa), P(oa), P(out_len), P(score)) == S.E_TOO_LARGE


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_align_long", "sw_align_long"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = _batch([(b"ACGT", b"ACG")])
    fn = getattr(ctx, call)
    extra = (0,) if call == "sw_align_long" else ()
    with pytest.raises(S.SeqAlignError) as e:
        fn(b, sc, *extra)                               # valid arguments reach the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "align_long" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        fn(b, {"preset": "default"}, *extra)            # not a scoring_t
    assert e.value.code == S.E_ARG
    with pytest.raises(S.SeqAlignError) as e:
        fn(W.Batch(b.arena, b.off_a.astype(np.int64), b.len_a, b.off_b, b.len_b), sc, *extra)   # offsets of the wrong type
    assert e.value.code == S.E_ARG
    if call == "sw_align_long":
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, [1, 2, 3])                        # min_score: one per pair
        assert e.value.code == S.E_ARG
