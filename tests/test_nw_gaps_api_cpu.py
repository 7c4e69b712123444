"""CPU tier: the surface of the NW gap-run calls (seqalign_nw_gaps_batch / _cross / _banded / _banded_wide and the two timing
hooks) -- exported and declared symbols, the wrappers, the unchanged kernel kind tables, and the argument checks of the C calls,
which are the nw_stats calls' of the same geometry in their order: every bad call is made on both siblings and must give one
status and one message.  All before any device is looked for: the context handed in is never dereferenced."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import seqalign_amd as S
from seqalign_amd import workloads as W

BATCH, CROSS, NARROW, WIDE = "seqalign_nw_gaps_batch", "seqalign_nw_gaps_cross", "seqalign_nw_gaps_banded", "seqalign_nw_gaps_banded_wide"
TIME, BAND_TIME = "seqalign_nw_gaps_time_ms", "seqalign_nw_gaps_band_time_ms"
SYMBOLS = [BATCH, CROSS, NARROW, WIDE, TIME, BAND_TIME]
HEADER = S.PKG_ROOT.parent / "include" / "seqalign_hip.h"
FULL = 2 ** 32 - 1


def twin(name):
    return name.replace("nw_gaps", "nw_stats")


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
    for f in ("nw_gaps", "nw_gaps_cross", "nw_gaps_banded", "nw_gaps_banded_wide", "nw_gaps_time_ms", "nw_gaps_band_time_ms"):
        assert callable(getattr(S.Context, f)), f
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in SYMBOLS:                               # the statistics calls' argument lists, word for word but for the outputs' names
        assert _decl(text, name) == _decl(text, twin(name)), name
    raw = HEADER.read_text()
    for out in ("out_gap_runs_a", "out_gap_runs_b"):
        assert raw.count(out) >= 8, out                # four NW calls beside the three SW ones
    assert not re.search(r"#define\s+SEQALIGN_\w*GAPS\w*", text)                    # no constant of their own


def test_kind_tables_are_unchanged():
    """The calls add no kind: the first table still ends at SEQALIGN_K_MAX (full), the second still names exactly three."""
    lib = S.lib()
    first = [lib.seqalign_kernel_kind_name(C.c_int(k)) for k in range(S.K_MAX + 1)]
    assert all(first[:S.K_MAX]) and first[S.K_MAX] is None
    second = [lib.seqalign_kernel_kind_ext_name(C.c_int(k)) for k in range(S.KX_MAX)]
    assert second[:3] == [b"band_score", b"band_fill", b"band_walk"] and not any(second[3:])


def _args(pairs, band):
    b = W.from_pairs(pairs)
    n = b.n_pairs
    q = W.seqset_from([a for a, _ in pairs])
    t = W.seqset_from([x for _, x in pairs])
    return dict(b=b, d=S.batch_desc(b), q=q, t=t, dq=S.seqset_desc(q), dt=S.seqset_desc(t), sc=S.make_scoring({"preset": "default"}),
                band=np.asarray(band, np.uint32), os=np.zeros(n * n, np.int32), u=[np.zeros(n * n, np.uint32) for _ in range(2)],
                ms=np.zeros(1, np.float32))


def _call_args(name, k, ctx, d=None):
    P = S._ptr
    head = [ctx, C.byref(d if d is not None else k["d"]), C.byref(k["sc"])]
    outs = [P(k["os"]), *[P(x) for x in k["u"]]]
    return {BATCH: head + outs, NARROW: head + [P(k["band"])] + outs, WIDE: head + [P(k["band"])] + outs,
            CROSS: [ctx, C.byref(k["dq"]), C.byref(k["dt"]), C.byref(k["sc"])] + outs,
            TIME: head + [C.c_int(1), P(k["ms"])],
            BAND_TIME: head + [P(k["band"]), C.c_int(1), P(k["ms"])]}[name.replace("nw_stats", "nw_gaps")]


def _call(lib, name, k, ctx, d=None):
    return getattr(lib, name)(*_call_args(name, k, ctx, d)), lib.seqalign_last_error().decode()


def _both(lib, name, k, ctx, d=None):
    """The call and its nw_stats twin on the same arguments: one status, one message."""
    got = _call(lib, name, k, ctx, d)
    assert got == _call(lib, twin(name), k, ctx, d), (name, got)
    return got


@pytest.mark.parametrize("name", SYMBOLS)
def test_c_calls_refuse_null_and_bad_arguments_without_a_device(name):
    lib = S.lib()
    k = _args([(b"ACGT", b"ACG"), (b"", b"T")], [1, 0])
    null, fake = C.c_void_p(0), C.c_void_p(1)      # `fake` is never dereferenced: every case fails first
    args = _call_args(name, k, fake)
    assert len(args) == {BATCH: 6, CROSS: 7, NARROW: 7, WIDE: 7, TIME: 5, BAND_TIME: 6}[name]
    for i, arg in enumerate(args):
        if isinstance(arg, C.c_int):
            continue
        bad = list(args)
        bad[i] = null
        assert getattr(lib, name)(*bad) == S.E_ARG, i
        assert getattr(lib, twin(name))(*bad) == S.E_ARG, i
    if name in (TIME, BAND_TIME):                  # repeats <= 0
        bad = list(args)
        bad[-2] = C.c_int(0)
        assert getattr(lib, name)(*bad) == S.E_ARG
    if name == CROSS:
        return
    b = k["b"]
    unreadable = S.BatchDesc(2, b.arena.ctypes.data, b.arena.nbytes, 0, b.len_a.ctypes.data, b.off_b.ctypes.data, b.len_b.ctypes.data)
    assert _both(lib, name, k, fake, unreadable)[0] == S.E_ARG      # refused before the context is touched
    if name in (TIME, BAND_TIME):                  # an empty batch
        e = _args([], [])
        assert _both(lib, name, e, fake)[0] == S.E_ARG


def _lengths_only(la, lb):
    arena = np.zeros(16, np.uint8)
    off = np.zeros(len(la), np.uint64)
    la, lb = np.asarray(la, np.uint32), np.asarray(lb, np.uint32)
    return (arena, off, la, lb), S.BatchDesc(len(la), arena.ctypes.data, arena.nbytes, off.ctypes.data, la.ctypes.data,
                                             off.ctypes.data, lb.ctypes.data)


@pytest.mark.parametrize("w, width", [(256, 513), (512, 1025), (FULL, 10000)])
def test_a_band_of_513_diagonals_is_refused_by_the_narrow_call_only(w, width):
    lib, fake, null = S.lib(), C.c_void_p(1), C.c_void_p(0)
    keep, d = _lengths_only([5000, 5000], [4999, 5000 if w != FULL else 4999])
    k = _args([(b"A", b"A")] * 2, [255, w])
    for name in (NARROW, BAND_TIME):
        rc, msg = _both(lib, name, k, fake, d)
        assert rc == S.E_TOO_LARGE and msg.startswith("pair 1:") and str(width) in msg, (name, rc, msg)
    rc, msg = _both(lib, WIDE, k, null, d)         # every check passed: the NULL context is what is refused
    assert rc == S.E_ARG, (rc, msg)
    k512 = _args([(b"A", b"A")] * 2, [255, 255])
    _, d512 = _lengths_only([5000, 5000], [4999, 4999])
    assert _both(lib, NARROW, k512, null, d512)[0] == S.E_ARG     # 512 diagonals: legal
    del keep


def test_no_length_limit_of_their_own():
    """Descriptors of 70 000 and 200 000 letters pass every check (the counts are full words): with nothing to refuse the call
    goes on to the context, NULL here."""
    lib, null = S.lib(), C.c_void_p(0)
    keep, d = _lengths_only([65536, 5, 70000], [5, 65536, 200000])
    k = _args([(b"A", b"A")] * 3, [3, 3, 3])
    for name in (BATCH, TIME, WIDE):
        rc, msg = _both(lib, name, k, null, d)
        assert rc == S.E_ARG, (name, rc, msg)
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
    for fn, sym in ((ctx.nw_gaps, BATCH), (ctx.nw_gaps_time_ms, TIME)):
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, sc)                                             # valid arguments reach the C call, which refuses the NULL context
        assert e.value.code == S.E_ARG and sym in str(e.value)
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, {"preset": "default"})
        assert e.value.code == S.E_ARG
        with pytest.raises(S.SeqAlignError):
            fn(object(), sc)
    with pytest.raises(S.SeqAlignError) as e:
        ctx.nw_gaps_time_ms(b, sc, repeats=0)
    assert e.value.code == S.E_ARG and "repeats" in str(e.value)
    q = W.seqset_from([b"ACGT", b"AC"])
    with pytest.raises(S.SeqAlignError) as e:
        ctx.nw_gaps_cross(q, q, sc)
    assert e.value.code == S.E_ARG and CROSS in str(e.value)
    with pytest.raises(S.SeqAlignError):
        ctx.nw_gaps_cross(b, q, sc)
    for fn, sym in ((ctx.nw_gaps_banded, NARROW), (ctx.nw_gaps_banded_wide, WIDE), (ctx.nw_gaps_band_time_ms, BAND_TIME)):
        for band in (3, [3, 0], np.array([5, 7], np.int64), FULL):
            with pytest.raises(S.SeqAlignError) as e:
                fn(b, sc, band)
            assert e.value.code == S.E_ARG and sym in str(e.value)
        for band in ([1, 2, 3], 1.5, "3", None, 2 ** 32, -1, [[1, 2]]):
            with pytest.raises(S.SeqAlignError) as e:
                fn(b, sc, band)
            assert e.value.code == S.E_ARG and "band:" in str(e.value), band
        with pytest.raises(S.SeqAlignError) as e:
            fn(b, {"preset": "default"}, 1)
        assert e.value.code == S.E_ARG
    with pytest.raises(S.SeqAlignError) as e:
        ctx.nw_gaps_band_time_ms(b, sc, 1, repeats=0)
    assert e.value.code == S.E_ARG and "repeats" in str(e.value)
