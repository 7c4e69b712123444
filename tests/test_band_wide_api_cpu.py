"""CPU tier: the wide banded calls' surface -- exported and declared symbols, the refusals that remain (E_ARG, E_TOO_LARGE
from lengths alone) and the Python wrappers' checks, all before any device is looked for: the context handed in is never
dereferenced.  The narrow calls' cap stays where it is."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

CALLS = ["seqalign_nw_score_banded_wide", "seqalign_nw_align_banded_wide", "seqalign_sw_score_banded_wide",
         "seqalign_sw_align_banded_wide"]
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"


def test_wide_symbols_are_exported_and_declared():
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


def test_the_narrow_cap_and_the_new_option_are_documented():
    header = HEADER.read_text()
    assert re.search(r"#define\s+SEQALIGN_BAND_MAX_WIDTH\s+1024\b", header)
    assert S.OPTION_DEFAULTS["band_strip_cols"] == 0
    assert "band_strip_cols" in header and "seqalign_nw_score_banded_wide" in header
    for method in ("nw_score_banded_wide", "nw_align_banded_wide", "sw_score_banded_wide", "sw_align_banded_wide"):
        assert callable(getattr(S.Context, method))


def _args(pairs):
    b = W.from_pairs(pairs)
    n = b.n_pairs
    return dict(b=b, d=S.batch_desc(b), sc=S.make_scoring({"preset": "default"}), band=np.full(n, 3, np.uint32),
                lo=np.full(n, -1, np.int32), hi=np.full(n, 1, np.int32), ms=np.ones(n, np.int32), hits=(S.SwHit * n)(),
                nh=C.c_uint64(7), oa=np.zeros(4096, np.uint8), ob=np.zeros(4096, np.uint8), os=np.zeros(n, np.int32),
                so=np.zeros(n, np.uint64), ol=np.zeros(n, np.uint32), ea=np.zeros(n, np.uint32), eb=np.zeros(n, np.uint32))


def _call_args(name, k, ctx):
    """(the call's arguments, the positions that are pointers)"""
    P = S._ptr
    head = [ctx, C.byref(k["d"]), C.byref(k["sc"])]
    if name == "seqalign_nw_score_banded_wide":
        return head + [P(k["band"]), P(k["os"])], range(5)
    if name == "seqalign_nw_align_banded_wide":
        return head + [P(k["band"]), P(k["so"]), P(k["oa"]), P(k["ob"]), P(k["ol"]), P(k["os"])], range(9)
    if name == "seqalign_sw_score_banded_wide":
        return head + [P(k["lo"]), P(k["hi"]), P(k["os"]), P(k["ea"]), P(k["eb"])], range(8)
    return head + [P(k["lo"]), P(k["hi"]), P(k["ms"]), k["hits"], C.c_uint64(len(k["hits"])), C.byref(k["nh"]), P(k["oa"]),
                   P(k["ob"]), C.c_uint64(4096)], (0, 1, 2, 3, 4, 5, 6, 8, 9, 10)      # 7 and 11 are the capacities


@pytest.mark.parametrize("name", CALLS)
def test_c_calls_refuse_null_arguments_and_unreadable_batches_without_a_device(name):
    lib = S.lib()
    fn = getattr(lib, name)
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args, pointers = _call_args(name, k, fake)
    for i in pointers:
        bad = list(args)
        bad[i] = null
        assert fn(*bad) == S.E_ARG, i
    # an unreadable batch: no off_a
    b = k["b"]
    bad = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    args[1] = C.byref(bad)
    assert fn(*args) == S.E_ARG


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


@pytest.mark.parametrize("name", CALLS[2:])
def test_sw_calls_refuse_crossed_bounds_without_a_device(name):
    """diag_lo > diag_hi as given: E_ARG with the pair named, wide bands before it accepted on the way."""
    lib, fake = S.lib(), C.c_void_p(1)
    keep, d = _lengths_only([5000, 100, 100], [5000, 90, 90])
    k = _args([(b"A", b"A")] * 3)
    k["lo"][:], k["hi"][:] = [-2000, 4, 200], [2000, 3, 150]      # pair 0: 4 001 diagonals
    args, _ = _call_args(name, k, fake)
    args[1] = C.byref(d)
    assert getattr(lib, name)(*args) == S.E_ARG
    assert lib.seqalign_last_error().decode().startswith("pair 1:")
    if name.endswith("align_banded_wide"):
        assert k["nh"].value == 0                  # the align call zeroes *n_hits before it looks at anything
    del keep


@pytest.mark.parametrize("name", CALLS)
def test_c_calls_refuse_a_pair_of_2_31_letters_from_lengths_alone(name):
    """The only E_TOO_LARGE left: pair 0's band of 3 001 (NW) / 4 001 (SW) diagonals is accepted, pair 1 is too long."""
    lib, fake = S.lib(), C.c_void_p(1)
    keep, d = _lengths_only([5000, 2 ** 30], [5000, 2 ** 30])
    k = _args([(b"A", b"A")] * 2)
    k["band"][:] = [1500, 0]
    k["lo"][:], k["hi"][:] = [-2000, 0], [2000, 0]
    args, _ = _call_args(name, k, fake)
    args[1] = C.byref(d)
    assert getattr(lib, name)(*args) == S.E_TOO_LARGE
    msg = lib.seqalign_last_error().decode()
    assert msg.startswith("pair 1:") and "2^31" in msg, msg
    del keep


def _deviceless_context():
    ctx = object.__new__(S.Context)   # a handle of NULL: the library answers E_ARG before it looks for a device
    ctx._h = C.c_void_p(0)
    ctx.device = 0
    return ctx


@pytest.mark.parametrize("call", ["nw_score_banded_wide", "nw_align_banded_wide"])
def test_nw_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    fn = getattr(ctx, call)
    for band in (3, [3, 0], np.array([1, 2 ** 31], np.uint32)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, band)                               # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and "banded_wide" in str(e.value)
    for band in ([1, 2, 3], -1, [0, -2], 1.5, "3", None, 2 ** 32, [[1, 2]]):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, band)
        assert e.value.code == S.E_ARG and "band:" in str(e.value), band
    with pytest.raises(S.SeqAlignError) as e:
        fn(b, {"preset": "default"}, 3)                   # not a scoring_t
    assert e.value.code == S.E_ARG


@pytest.mark.parametrize("call", ["sw_score_banded_wide", "sw_align_banded_wide"])
def test_sw_wrappers_check_their_arguments(call):
    ctx = _deviceless_context()
    sc = S.make_scoring({"preset": "default"})
    b = W.from_pairs([(b"ACGT", b"ACG"), (b"AC", b"ACT")])
    tail = (1,) if call == "sw_align_banded_wide" else ()
    fn = getattr(ctx, call)
    for lo, hi in ((-3, 3), ([-3, 0], [3, 0]), (-2 ** 31, 2 ** 31 - 1)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, lo, hi, *tail)                      # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and "banded_wide" in str(e.value)
    for lo in ([1, 2, 3], 1.5, "3", None, 2 ** 31, [[1, 2]]):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, lo, 2 ** 31 - 1, *tail)
        assert e.value.code == S.E_ARG and "diag_lo:" in str(e.value), lo
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, -5, lo, *tail)
        assert e.value.code == S.E_ARG and "diag_hi:" in str(e.value), lo
    if call == "sw_align_banded_wide":
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc, -1, 1, [1, 2, 3])
        assert e.value.code == S.E_ARG and "min_score" in str(e.value)
