"""CPU tier: the banded calls' surface -- exported and declared symbols, the second launch record's kind names, the argument
checks of the C calls (E_ARG, E_TOO_LARGE) and of the Python wrappers, all before any device is looked for."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

CALLS = ["seqalign_nw_score_banded", "seqalign_nw_align_banded", "seqalign_band_score_time_ms"]
EXT = ["seqalign_ctx_last_call_info_ext", "seqalign_kernel_kind_ext_name"]
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"

OLD_KINDS = [b"fill_wavefront", b"fill_rowscan", b"fill_stream", b"fill_strips", b"fill_wgstream", b"fill_nw_dirs",
             b"fill_nw_dirs_x2", b"fill_sw_dirs", b"fill_sw_dirs_x2", b"fill_sw_best_x2", b"sw_reduce", b"sw_box", b"sweep_regs",
             b"sweep_lds", b"sweep_strips", b"sweep_dirs", b"sweep_dirs_x2", b"walk_lane", b"walk_wave", b"walk_dirs_lane",
             b"walk_dirs_tile", b"walk_moves_lane", b"walk_moves_tile", b"fill_nw_dirs_x4", b"fill_sw_best_x4", b"score_rows",
             b"score_strips", b"score_cross", b"score_select", b"long_forward", b"long_block", b"long_walk"]


def test_band_symbols_are_exported_and_declared():
    out = subprocess.run(["nm", "-D", "--defined-only", str(S.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(CALLS + EXT) <= defined, set(CALLS + EXT) - defined
    assert set(CALLS + EXT) <= set(S.EXPORTED_SYMBOLS)
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in CALLS + EXT:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+SEQALIGN_BAND_MAX_WIDTH\s+1024\b", text)
    assert "seqalign_call_info_ext_t" in text


def test_ext_kind_names_and_the_old_table():
    lib = S.lib()
    names = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(-1, S.KX_MAX + 1)]
    assert names[0] is None
    assert names[1:4] == [b"band_score", b"band_fill", b"band_walk"]
    assert all(n is None for n in names[4:])
    # the first record is ABI and full: its 32 names are what they were
    assert [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX)] == OLD_KINDS
    assert lib.seqalign_kernel_kind_name(C.c_int(S.K_MAX)) is None
    assert C.sizeof(S.CallInfoExt) == C.sizeof(S.CallInfo) == 32 * 4 + 32 * 8
    assert lib.seqalign_ctx_last_call_info_ext(C.c_void_p(0), C.byref(S.CallInfoExt())) == S.E_ARG


def _args(pairs, band):
    b = W.from_pairs(pairs)
    n = b.n_pairs
    keep = dict(b=b, d=S.batch_desc(b), sc=S.make_scoring({"preset": "default"}), band=np.asarray(band, np.uint32),
                so=np.zeros(n, np.uint64), oa=np.zeros(4096, np.uint8), ob=np.zeros(4096, np.uint8),
                ol=np.zeros(n, np.uint32), os=np.zeros(n, np.int32))
    caps = b.len_a.astype(np.uint64) + b.len_b.astype(np.uint64) + np.uint64(1)
    keep["so"][1:] = np.cumsum(caps)[:-1]
    return keep


def test_c_calls_refuse_null_arguments_without_a_device():
    lib, P = S.lib(), S._ptr
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")], [1, 0])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    score_args = [fake, C.byref(k["d"]), C.byref(k["sc"]), P(k["band"]), P(k["os"])]
    for i in range(len(score_args)):
        args = list(score_args)
        args[i] = null
        assert lib.seqalign_nw_score_banded(*args) == S.E_ARG, i
    align_args = [fake, C.byref(k["d"]), C.byref(k["sc"]), P(k["band"]), P(k["so"]), P(k["oa"]), P(k["ob"]), P(k["ol"]), P(k["os"])]
    for i in range(len(align_args)):
        args = list(align_args)
        args[i] = null
        assert lib.seqalign_nw_align_banded(*args) == S.E_ARG, i
    ms = np.zeros(4, np.float32)
    time_args = [fake, C.byref(k["d"]), C.byref(k["sc"]), P(k["band"]), C.c_int(4), P(ms)]
    for i in (0, 1, 2, 3, 5):
        args = list(time_args)
        args[i] = null
        assert lib.seqalign_band_score_time_ms(*args) == S.E_ARG, i
    for repeats in (0, -3):
        assert lib.seqalign_band_score_time_ms(*time_args[:4], C.c_int(repeats), P(ms)) == S.E_ARG, repeats
    b = k["b"]
    bad = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert lib.seqalign_nw_score_banded(fake, C.byref(bad), C.byref(k["sc"]), P(k["band"]), P(k["os"])) == S.E_ARG
    assert lib.seqalign_nw_align_banded(fake, C.byref(bad), *align_args[2:]) == S.E_ARG
    assert lib.seqalign_band_score_time_ms(fake, C.byref(bad), *time_args[2:]) == S.E_ARG


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


def test_c_calls_refuse_a_band_of_1025_diagonals_without_a_device():
    """Found from the lengths and the bands alone: the sequences are not read, no device is looked for, the pair is named."""
    lib, P = S.lib(), S._ptr
    sc = S.make_scoring({"preset": "default"})
    fake = C.c_void_p(1)
    # pair 0: 1 + 1 + 2 * 511 = 1 024 diagonals (legal); pair 1: 600 + 1 + 2 * 212 = 1 025
    keep, d = _lengths_only([5000, 5000], [4999, 4400])
    band = np.array([511, 212], np.uint32)
    so, ol, os_ = np.zeros(2, np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.int32)
    oa = np.zeros(8, np.uint8)
    assert lib.seqalign_nw_score_banded(fake, C.byref(d), C.byref(sc), P(band), P(os_)) == S.E_TOO_LARGE
    assert lib.seqalign_last_error().decode().startswith("pair 1:") and "1025" in lib.seqalign_last_error().decode()
    assert lib.seqalign_nw_align_banded(fake, C.byref(d), C.byref(sc), P(band), P(so), P(oa), P(oa), P(ol), P(os_)) == S.E_TOO_LARGE
    assert lib.seqalign_last_error().decode().startswith("pair 1:")
    ms = np.zeros(2, np.float32)
    assert lib.seqalign_band_score_time_ms(fake, C.byref(d), C.byref(sc), P(band), C.c_int(2), P(ms)) == S.E_TOO_LARGE
    # a pair whose own shape needs more diagonals than that, whatever the band
    keep2, d2 = _lengths_only([300], [2000000])
    zero = np.zeros(1, np.uint32)
    assert lib.seqalign_nw_score_banded(fake, C.byref(d2), C.byref(sc), P(zero), P(os_)) == S.E_TOO_LARGE
    assert lib.seqalign_nw_align_banded(fake, C.byref(d2), C.byref(sc), P(zero), P(so), P(oa), P(oa), P(ol), P(os_)) == S.E_TOO_LARGE
    del keep, keep2


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_score_banded", "nw_align_banded"])
def test_python_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    fn = getattr(ctx, call)
    for band in (3, [3, 0], np.array([1, 2 ** 31], np.uint32)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, band)                               # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and "banded" in str(e.value)
    for band in ([1, 2, 3], -1, [0, -2], 1.5, "3", None, 2 ** 32, [[1, 2]]):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, band)
        assert e.value.code == S.E_ARG and "band:" in str(e.value), band
    with pytest.raises(S.SeqAlignError) as e:
        fn(b, {"preset": "default"}, 3)                   # not a scoring_t
    assert e.value.code == S.E_ARG
    with pytest.raises(S.SeqAlignError) as e:
        fn(W.Batch(b.arena, b.off_a.astype(np.int64), b.len_a, b.off_b, b.len_b), sc, 3)   # offsets of the wrong type
    assert e.value.code == S.E_ARG


def test_timing_hook_wrapper_checks_its_arguments():
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    with pytest.raises(S.SeqAlignError) as e:
        ctx.band_score_time_ms(b, sc, 3, repeats=2)       # reaches the C call, which refuses the NULL context
    assert e.value.code == S.E_ARG and "seqalign_band_score_time_ms" in str(e.value)
    with pytest.raises(S.SeqAlignError) as e:
        ctx.band_score_time_ms(b, sc, [1, 2, 3])
    assert e.value.code == S.E_ARG and "band:" in str(e.value)
