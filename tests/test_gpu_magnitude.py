"""GPU tier: every int32 kernel at large score magnitudes (tests/maglib.py: scorings multiplied by a scale, small pairs).

Every other GPU test draws a match of 1 .. 6 and penalties no lower than -13; here the cells stand between 2^15 and 2^31.  Each
family of maglib.FAMILIES runs through every call family on every shape -- one batch per (family, shape, NW | SW): an identical
pair, a disjoint one, one planted gap each way (and, on the square shape, both) -- and everything is compared with the oracle,
field for field and byte for byte (tests/test_magnitude_argument_cpu.py argues on the CPU that the inputs are defined upstream
and reach their magnitudes).

The row sweeps de-trend gap_b (sa_rowsweep.hpp), which adds up to a frame's width of gap_extend to a cell: sums the reference
never forms.  The library refuses, before any launch and with SEQALIGN_E_DOMAIN, the scorings whose documented bound
(include/seqalign_hip.h; maglib.admitted restates it independently) leaves int32 there; the tests assert the reference's
result on one side of that bound and the refusal on the other, for every call.
"""
import numpy as np
import pytest

import bandlib as BL
import bandspanlib as BSP
import bandswlib as BS
import denselib as D
import maglib as G
import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

KERNELS = [S.KERNEL_WAVEFRONT, S.KERNEL_ROWSCAN, S.KERNEL_STREAM, S.KERNEL_STRIPS, S.KERNEL_WGSTREAM]
FAMS = pytest.mark.parametrize("fam", G.FAMILIES, ids=G.family_id)
FAMS_SW = pytest.mark.parametrize("fam", [f for f in G.FAMILIES if f[0] not in G.FLOOR_BASES], ids=G.family_id)      # the floor families are NW only
PACKED = ("fill_nw_dirs_x2", "fill_nw_dirs_x4", "fill_sw_dirs_x2", "fill_sw_best_x2", "fill_sw_best_x4", "sweep_dirs_x2")
STRIP = 64
LONG_ROWS = 8           # three blocks at len_b = 24, twelve at 96
DIRS_PAIRS = 384        # from here on the directions-only NW fill takes rows of 769 .. 1 024 columns


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


_SC, _WANT = {}, {}


def scoring(spec):
    key = repr(spec)
    if key not in _SC:
        _SC[key] = S.make_scoring(spec)
    return _SC[key]


def want(kind, c, *args):
    """The oracle's answer, once per (case, question) for the whole file."""
    key = (kind, c.id, args)
    if key not in _WANT:
        osc = c.osc()
        if kind == "fill":
            rc, M, A, B = O.oracle_fill(osc, c.a, c.b, c.is_sw)
            assert rc == 0
            v = (M, A, B)
        elif kind == "nw":
            rc, s, ra, rb = O.oracle_nw(osc, c.a, c.b)
            assert rc == 0
            v = (s, ra, rb)
        elif kind == "sw":
            rc, v = O.oracle_sw(osc, c.a, c.b, *args)
            assert rc == 0
        elif kind == "nw_band":
            v = BL.expected_both(osc, c.a, c.b, *args)
        elif kind == "sw_band":
            cell, fields = BSP.want(osc, c.a, c.b, *args)
            v = (cell, fields, BS.expected(osc, c.a, c.b, *args, thr(c))[1])
        _WANT[key] = v
    return _WANT[key]


def thr(c):
    """min_score of the SW calls: four matches."""
    return 4 * c.spec["init"][0]


class Tally:
    """Collects what went wrong over a test's calls, so that one run names every call that differs."""

    def __init__(self):
        self.bad, self.exact, self.refused = [], 0, 0

    def attempt(self, label, admitted, call, verify):
        try:
            got = call()
        except S.SeqAlignError as e:
            if admitted or e.code != S.E_DOMAIN or str(G.INT32_MAX) not in str(e):
                self.bad.append((label, f"raised {str(e)[:160]}"))
            else:
                self.refused += 1
            return
        if not admitted:
            self.bad.append((label, "no SEQALIGN_E_DOMAIN for a scoring outside the documented bound"))
            return
        msg = verify(got)
        if msg:
            self.bad.append((label, msg))
        else:
            self.exact += 1

    def done(self, what):
        print(f"{what}: {self.exact} calls equal to the oracle, {self.refused} refused with E_DOMAIN")
        assert not self.bad, (len(self.bad), self.bad[:12])
        assert self.exact + self.refused > 0


def group_of(fam, is_sw=None):
    for _, shape, sw, cs in G.groups(fam, is_sw):
        la, lb = G.group_lengths(cs)
        yield shape, sw, cs, W.from_pairs([(c.a, c.b) for c in cs]), scoring(cs[0].spec), la, lb


def first_diff(got, wanted):
    bad = [p for p, (g, w) in enumerate(zip(got, wanted)) if g != w]
    return None if not bad and len(got) == len(wanted) else f"pairs {bad[:6]} differ: got {got[bad[0]] if bad else len(got)}, oracle {wanted[bad[0]] if bad else len(wanted)}"


# ------------------------------------------------------------------------------------------- A. the device-level fills ---
@FAMS
def test_device_fills_every_kernel(ctx, fam):
    """seqalign_fill_batch_device with each of the five kernels: M, A and B of every pair, every cell."""
    import torch
    t = Tally()
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
        adm = G.admitted(cs[0].spec, la, lb, "fill")
        db = S.DeviceBatch(batch, 0, placement="packed", ctx=ctx)
        h = ctx.upload_scoring(sc, is_sw)
        for kernel in KERNELS:
            def call():
                for x in (db.M, db.A, db.B):
                    x.fill_(0x5A5A5A5A)
                db.fill(ctx, h, kernel)
                torch.cuda.synchronize()
                return [db.pair_matrices(p) for p in range(len(cs))]

            def verify(got):
                for c, g in zip(cs, got):
                    for name, x, w in zip("MAB", g, want("fill", c)):
                        if not np.array_equal(x, w):
                            k = int(np.nonzero(x != w)[0][0])
                            return f"{c.kind} {name} cell {k} (i={k % (len(c.a) + 1)}, j={k // (len(c.a) + 1)}): gpu {x[k]} oracle {w[k]}"
                if (db.status.cpu().numpy() != -1).any():
                    return "status"
            t.attempt((shape, is_sw, S.KERNEL_NAMES[kernel]), adm, call, verify)
        ctx.release_scoring(h)
    t.done(G.family_id(fam))


def test_host_fill_batch(ctx):
    """seqalign_fill_batch (upload, fill, download) on the top and floor families."""
    t = Tally()
    for fam in [f for f in G.FAMILIES if f[1] in (G.TOP, 29)]:
        for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
            def verify(got):
                M, A, B, off, status = got
                for p, c in enumerate(cs):
                    o, n = int(off[p]), (len(c.a) + 1) * (len(c.b) + 1)
                    if not all(np.array_equal(X[o:o + n], w) for X, w in zip((M, A, B), want("fill", c))):
                        return f"{c.kind} differs"
            t.attempt((G.family_id(fam), shape, is_sw), G.admitted(cs[0].spec, la, lb, "fill"),
                      lambda: ctx.fill_batch(batch, sc, is_sw), verify)
    t.done("fill_batch")


# ------------------------------------------------------------------------------------------------------- B. nw_batch ---
NW_ROUTES = (("dirs", dict(nw_dirs=1, pack16=2)), ("dirs-strings", dict(nw_dirs=1, nw_moves=0)), ("matrices", dict(nw_dirs=0)),
             ("host", dict(traceback="host")))


@FAMS
def test_nw_batch_every_route(ctx, fam):
    """seqalign_nw_batch through the directions-only fill (pack16 = 2: the packed int16 fills must still decline), the same
    with strings sent home, the three-matrix fill with device walks, and host traceback; one CIGAR route.  The shape of 1 001
    columns runs as 384 pairs, where the directions-only fill takes such rows."""
    t = Tally()
    plain = not G.BASES[fam[0]]["init"][4:9].count(1) and G.BASES[fam[0]]["init"][3] <= 0 and G.BASES[fam[0]]["init"][2] <= 0
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam, 0):
        adm = G.admitted(cs[0].spec, la, lb, "fill")
        wanted = [want("nw", c) for c in cs]
        reps = -(-DIRS_PAIRS // len(cs)) if shape == "c16" else 1
        for route, options in NW_ROUTES:
            many = reps if route.startswith("dirs") else 1
            b = W.from_pairs([(c.a, c.b) for c in cs] * many) if many > 1 else batch
            with ctx.options(**options):
                def call():
                    got = ctx.nw_batch(b, sc)
                    return got, ctx.last_call()

                def verify(res):
                    got, ran = res
                    if set(ran) & set(PACKED):
                        return f"a packed int16 fill ran: {ran}"
                    if route.startswith("dirs") and plain and shape != "strips" and "fill_nw_dirs" not in ran:
                        return f"not the directions-only fill: {ran}"
                    if route == "matrices" and "fill_nw_dirs" in ran:
                        return f"not the three-matrix fill: {ran}"
                    return first_diff(got, wanted * many)
                t.attempt((shape, route), adm, call, verify)
        t.attempt((shape, "cigar"), adm, lambda: ctx.nw_batch_cigar(batch, sc, fmt=D.EQX),
                  lambda got: first_diff(got, [(s, D.cigar(ra, rb, D.EQX).encode()) for s, ra, rb in wanted]))
    t.done(G.family_id(fam))


# ------------------------------------------------------------------------------------------------------- C. sw_batch ---
SW_ROUTES = (("dirs-ev", dict(sweep_dirs=1, sweep_ev=1, pack16=2)), ("dirs", dict(sweep_dirs=1, sweep_ev=0)),
             ("matrices-pair", dict(sweep_dirs=0, sweep_mode="pair")), ("matrices-strips", dict(sweep_dirs=0, sweep_mode="strips")))


@FAMS_SW
def test_sw_batch_every_route(ctx, fam):
    """seqalign_sw_batch with max_hits 1 and 4 through the direction-byte fill and both forms of its sweep, and through the
    three-matrix fill with the sweep of one wave per pair and of strips."""
    t = Tally()
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam, 1):
        adm = G.admitted(cs[0].spec, la, lb, "fill")
        for max_hits in (1, 4):
            wanted = [want("sw", c, thr(c), max_hits) for c in cs]
            for route, options in SW_ROUTES:
                with ctx.options(**options):
                    def call():
                        got = ctx.sw_batch(batch, sc, thr(cs[0]), max_hits=max_hits)
                        return got, ctx.last_call()

                    def verify(res):
                        got, ran = res
                        if set(ran) & set(PACKED):
                            return f"a packed int16 fill ran: {ran}"
                        return first_diff(got, wanted)
                    t.attempt((shape, route, max_hits), adm, call, verify)
    t.done(G.family_id(fam))


# ------------------------------------------------------------------------------------------- D. score, span and cross ---
@FAMS
def test_score_and_span_calls(ctx, fam):
    """nw_score, sw_score and sw_span: rows of 1, 2, 8 and 16 columns per lane and the strips forms (sw_span from 513 columns
    on, the score calls at 1 101)."""
    t = Tally()
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
        adm = G.admitted(cs[0].spec, la, lb, "score")
        if not is_sw:
            t.attempt((shape, "nw_score"), adm, lambda: (ctx.nw_score(batch, sc).tolist(), ctx.last_call()),
                      lambda r: first_diff(r[0], [want("nw", c)[0] for c in cs]) or
                      (None if ("score_strips" in r[1]) == (la > 1024) else f"wrong form: {r[1]}"))
            continue
        hits = [want("sw", c, 1, 1) for c in cs]
        ends = [(h[0]["score"], h[0]["pos_a"] + h[0]["len_a"], h[0]["pos_b"] + h[0]["len_b"]) if h else (0, 0, 0) for h in hits]
        t.attempt((shape, "sw_score"), adm, lambda: [tuple(int(x[p]) for x in ctx.sw_score(batch, sc)) for p in range(len(cs))],
                  lambda got: first_diff(got, ends))
        t.attempt((shape, "sw_span"), adm, lambda: [tuple(int(x[p]) for x in ctx.sw_span(batch, sc)) for p in range(len(cs))],
                  lambda got: first_diff(got, [BSP.fields(h[0] if h else None) for h in hits]))
    t.done(G.family_id(fam))


@FAMS
def test_score_cross(ctx, fam):
    """nw_score_cross and sw_score_cross: every seq_a of a group against every seq_b."""
    t = Tally()
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
        adm = G.admitted(cs[0].spec, la, lb, "score")
        q, tg = W.seqset_from([c.a for c in cs]), W.seqset_from([c.b for c in cs])
        fills = [[O.oracle_fill(cs[0].osc(), x.a, y.b, is_sw) for y in cs] for x in cs]
        assert all(f[0] == 0 for row in fills for f in row)
        if is_sw:
            best = [[BS.best_cell(f[1], len(x.a)) for f in row] for x, row in zip(cs, fills)]
            t.attempt((shape, "sw_cross"), adm, lambda: ctx.sw_score_cross(q, tg, sc),
                      lambda got: None if [[(int(got[0][i, j]), int(got[1][i, j]), int(got[2][i, j])) for j in range(len(cs))]
                                           for i in range(len(cs))] == best else "differs")
        else:
            end = [[BL.end_value(*f[1:]) for f in row] for row in fills]
            t.attempt((shape, "nw_cross"), adm, lambda: ctx.nw_score_cross(q, tg, sc).tolist(),
                      lambda got: None if got == end else "differs")
    t.done(G.family_id(fam))


# --------------------------------------------------------------------------------------------------- E. the long calls ---
@FAMS
def test_align_long(ctx, fam):
    """nw_align_long and sw_align_long with blocks of 8 rows: three blocks at len_b = 24, twelve at 96."""
    t = Tally()
    with ctx.options(long_block_rows=LONG_ROWS):
        for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
            adm = G.admitted(cs[0].spec, la, lb, "score")

            def blocks(r):
                return None if r[1].get("long_block", (0, 0))[0] >= 3 else f"fewer than three blocks: {r[1]}"
            if is_sw:
                t.attempt((shape, "sw_long"), adm, lambda: (ctx.sw_align_long(batch, sc, thr(cs[0])), ctx.last_call()),
                          lambda r: first_diff(r[0], [want("sw", c, thr(c), 1) for c in cs]) or blocks(r))
            else:
                t.attempt((shape, "nw_long"), adm, lambda: (ctx.nw_align_long(batch, sc), ctx.last_call()),
                          lambda r: first_diff(r[0], [want("nw", c) for c in cs]) or blocks(r))
    t.done(G.family_id(fam))


# ------------------------------------------------------------------------------------------------- F. the banded calls ---
def sw_band_of(c, k):
    if c.kind in ("gapb", "gapa", "both"):
        return G.sw_bands(c.shape, c.kind)[k][:2]
    d = len(c.a) - len(c.b)
    return [(d - 1, d + 1), (d, d), (d - 3, d + 8)][k]


def nw_band_of(c, k):
    bands = G.nw_bands(c.shape, c.kind) if c.kind in ("gapb", "gapa", "both") else [(0, True), (1, True), (3, True)]
    return bands[k % len(bands)][0]


def same_status(narrow, wide):
    """Both raise the same code, or neither raises."""
    codes = []
    for fn in (narrow, wide):
        try:
            fn()
            codes.append(S.OK)
        except S.SeqAlignError as e:
            codes.append(e.code)
    return codes[0] == codes[1], codes


@FAMS
def test_banded_calls(ctx, fam):
    """The narrow banded calls, the wide ones at strips of 64 columns, and sw_span_banded, each pair under three bands of its
    own: for the planted pairs bands that hold the path and bands that cut it (maglib.sw_bands / nw_bands).  Narrow and wide
    agree on the status, refusals included."""
    t = Tally()
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
        adm = G.admitted(cs[0].spec, la, lb, "band")
        n = len(cs)
        for k in range(3):
            if is_sw:
                lo, hi = (np.array(v, np.int32) for v in zip(*[sw_band_of(c, k) for c in cs]))
                w = [want("sw_band", c, *sw_band_of(c, k)) for c in cs]
                cells, spans, hits = [x[0] for x in w], [x[1] for x in w], [[x[2]] if x[2] else [] for x in w]
                triple = lambda r: [tuple(int(x[p]) for x in r) for p in range(n)]
                t.attempt((shape, k, "sw_score_banded"), adm, lambda: triple(ctx.sw_score_banded(batch, sc, lo, hi)), lambda g: first_diff(g, cells))
                t.attempt((shape, k, "sw_align_banded"), adm, lambda: ctx.sw_align_banded(batch, sc, lo, hi, thr(cs[0])), lambda g: first_diff(g, hits))
                t.attempt((shape, k, "sw_span_banded"), adm, lambda: triple(ctx.sw_span_banded(batch, sc, lo, hi)), lambda g: first_diff(g, spans))
                with ctx.options(band_strip_cols=STRIP):
                    t.attempt((shape, k, "sw_score_banded_wide"), adm, lambda: triple(ctx.sw_score_banded_wide(batch, sc, lo, hi)), lambda g: first_diff(g, cells))
                    t.attempt((shape, k, "sw_align_banded_wide"), adm, lambda: ctx.sw_align_banded_wide(batch, sc, lo, hi, thr(cs[0])), lambda g: first_diff(g, hits))
                    ok, codes = same_status(lambda: ctx.sw_score_banded(batch, sc, lo, hi), lambda: ctx.sw_score_banded_wide(batch, sc, lo, hi))
                    assert ok, (shape, k, codes)
            else:
                bw = np.array([nw_band_of(c, k) for c in cs], np.uint32)
                w = [want("nw_band", c, nw_band_of(c, k)) for c in cs]
                scores, aligned = [x[0] for x in w], [x[1] for x in w]
                narrow = max(BL.width_of(len(c.a), len(c.b), int(v)) for c, v in zip(cs, bw)) <= 1024
                calls = [("nw_score_banded_wide", lambda: ctx.nw_score_banded_wide(batch, sc, bw).tolist(), scores)]
                if narrow:
                    calls.append(("nw_score_banded", lambda: ctx.nw_score_banded(batch, sc, bw).tolist(), scores))
                if None not in aligned:
                    calls.append(("nw_align_banded_wide", lambda: ctx.nw_align_banded_wide(batch, sc, bw), aligned))
                    if narrow:
                        calls.append(("nw_align_banded", lambda: ctx.nw_align_banded(batch, sc, bw), aligned))
                with ctx.options(band_strip_cols=STRIP):
                    for name, fn, wanted in calls:
                        t.attempt((shape, k, name), adm, fn, lambda g, wanted=wanted: first_diff(g, wanted))
                    if narrow:
                        ok, codes = same_status(calls[1][1], calls[0][1])
                        assert ok, (shape, k, codes)
    t.done(G.family_id(fam))
