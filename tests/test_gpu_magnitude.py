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

Sections G and H run the statistics calls, the span and statistics calls over sets and the banded statistics and span calls:
their payload sweeps carry counts and spans beside the values and decide on the values which payload a cell inherits.  The deep
families (NW only) put real scores into (-2^31, -2^30), below INT32_MIN / 2 and above the floor.
"""
import numpy as np
import pytest

import bandlib as BL
import bandnwstatlib as BN
import bandspanlib as BSP
import bandswlib as BS
import denselib as D
import maglib as G
import orclib as O
import statlib as ST
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

KERNELS = [S.KERNEL_WAVEFRONT, S.KERNEL_ROWSCAN, S.KERNEL_STREAM, S.KERNEL_STRIPS, S.KERNEL_WGSTREAM]
FAMS = pytest.mark.parametrize("fam", G.FAMILIES, ids=G.family_id)
FAMS_SW = pytest.mark.parametrize("fam", [f for f in G.FAMILIES if not G.nw_only(f)], ids=G.family_id)      # the floor and the deep families are NW only
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
        elif kind == "nw_stats":                # the oracle's score and the counted columns of its strings
            s, ra, rb = want("nw", c)
            v = (s,) + ST.count_columns(osc, ra, rb)
        elif kind == "sw_stats":                # the oracle's first hit at min_score = 1 and the counted columns of its strings
            v = stats_of(osc, (want("sw", c, 1, 1) or [None])[0])
        elif kind == "nw_band_stats":           # (the banded end value, its three statistics or None: no walk inside the band)
            value, walked = want("nw_band", c, *args)
            if walked is not None and BN.walked_along_the_floor(osc, c.a, c.b, *args, walked[1], walked[2]):
                walked = None                   # the documented family under no_mismatches: no alignment of the banded problem
            v = (value, None if walked is None else (walked[0],) + ST.count_columns(osc, walked[1], walked[2]))
        elif kind == "sw_band_stats":           # the banded hit at min_score = 1 and its counted strings
            v = stats_of(osc, BS.expected(osc, c.a, c.b, *args, 1)[1])
        _WANT[key] = v
    return _WANT[key]


def thr(c):
    """min_score of the SW calls: four matches."""
    return 4 * c.spec["init"][0]


def stats_of(osc, hit):
    """The seven words of the SW statistics calls for an oracle hit (or none): its five fields and its strings' counts."""
    return BSP.fields(hit) + (ST.count_columns(osc, hit["a"].encode(), hit["b"].encode()) if hit else (0, 0))


def want_set(cs, i, j, is_sw):
    """The oracle's answer for seq_a of case i against seq_b of case j of one group, once for the whole file: NW (score,
    matches, mismatches); SW the seven words of the first hit at min_score = 1."""
    key = ("set", cs[i].id, cs[j].id, is_sw)
    if key not in _WANT:
        osc = cs[0].osc()
        if is_sw:
            rc, hits = O.oracle_sw(osc, cs[i].a, cs[j].b, 1, 1)
            assert rc == 0
            _WANT[key] = stats_of(osc, hits[0] if hits else None)
        else:
            rc, score, ra, rb = O.oracle_nw(osc, cs[i].a, cs[j].b)
            assert rc == 0, key
            _WANT[key] = (score,) + ST.count_columns(osc, ra, rb)
    return _WANT[key]


# per call name, over the whole file: [calls equal to the oracle, calls refused with E_DOMAIN], and the families that ran
CALL_COUNTS, FAMILIES_RUN = {}, set()


class Tally:
    """Collects what went wrong over a test's calls, so that one run names every call that differs."""

    def __init__(self):
        self.bad, self.exact, self.refused = [], 0, 0

    def attempt(self, label, admitted, call, verify, name=None):
        """name: the call counted in CALL_COUNTS besides (results only: an expected SEQALIGN_E_TRACEBACK goes without)."""
        per_call = CALL_COUNTS.setdefault(name, [0, 0]) if name else [0, 0]
        try:
            got = call()
        except S.SeqAlignError as e:
            if admitted or e.code != S.E_DOMAIN or str(G.INT32_MAX) not in str(e):
                self.bad.append((label, f"raised {str(e)[:160]}"))
            else:
                self.refused += 1
                per_call[1] += 1
            return
        if not admitted:
            self.bad.append((label, "no SEQALIGN_E_DOMAIN for a scoring outside the documented bound"))
            return
        msg = verify(got)
        if msg:
            self.bad.append((label, msg))
        else:
            self.exact += 1
            per_call[0] += 1

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


# ------------------------------------------------------------------------- G. the statistics calls and the calls over sets ---
NEW_CALLS = ("nw_stats", "nw_stats_cross", "sw_stats", "sw_stats_cross", "sw_span_cross", "sw_span_search", "nw_stats_banded",
             "sw_stats_banded", "nw_stats_banded_wide", "sw_stats_banded_wide", "sw_span_banded_wide")


def rows_of(res, n):
    return [tuple(int(x[p]) for x in res) for p in range(n)]


def form_of(ran, la):
    """The payload sweeps (span, statistics) take a seq_a of up to 512 letters in one wave and strips beyond: the shapes of
    1 001 and of 1 101 columns run as strips, and nothing else does."""
    return None if set(ran) == ({"score_strips"} if la > 512 else {"score_rows"}) else f"wrong form: {ran}"


@FAMS
def test_stats_calls(ctx, fam):
    """nw_stats: the oracle's score and the counted columns of its strings; sw_stats: the five fields of the oracle's first hit
    at min_score = 1 and the counts of its strings.  One wave per pair up to 512 columns, strips beyond -- recorded as
    score_strips on the shape of 1 101 columns (and of 1 001), as score_rows on the others."""
    t = Tally()
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
        adm = G.admitted(cs[0].spec, la, lb, "score")
        name = "sw_stats" if is_sw else "nw_stats"
        wanted = [want(name, c) for c in cs]
        fn = ctx.sw_stats if is_sw else ctx.nw_stats
        t.attempt((shape, name), adm, lambda: (rows_of(fn(batch, sc), len(cs)), ctx.last_call()),
                  lambda r: first_diff(r[0], wanted) or form_of(r[1], la), name)
    FAMILIES_RUN.add(("stats", fam))
    t.done(G.family_id(fam))


def top_k(matrix, k, min_score):
    """The search calls' contract on an expected matrix of tuples (score first): per query the targets with score >= min_score,
    score descending then target ascending, the first k."""
    out = []
    for row in matrix:
        order = sorted((j for j, x in enumerate(row) if x[0] >= min_score), key=lambda j: (-row[j][0], j))[:k]
        out.append([(j,) + row[j][:5] for j in order])
    return out


@FAMS
def test_stats_and_span_over_sets(ctx, fam):
    """nw_stats_cross, sw_stats_cross and sw_span_cross: every seq_a of a group against every seq_b, from oracle fills and
    walks.  sw_span_search with k = 3 at min_score = 1 and at four matches: sw_score_search's order (score descending, then
    target ascending) over the expected matrix, spans taken from it."""
    t = Tally()
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
        adm = G.admitted(cs[0].spec, la, lb, "score")      # the longest query and the longest target
        n = len(cs)
        q, tg = W.seqset_from([c.a for c in cs]), W.seqset_from([c.b for c in cs])
        wanted = [[want_set(cs, i, j, is_sw) for j in range(n)] for i in range(n)]
        grid = lambda res: [[tuple(int(x[i, j]) for x in res) for j in range(n)] for i in range(n)]
        same = lambda w: lambda got: None if got == w else f"differs: got {got}, oracle {w}"
        if not is_sw:
            t.attempt((shape, "nw_stats_cross"), adm, lambda: grid(ctx.nw_stats_cross(q, tg, sc)), same(wanted), "nw_stats_cross")
            continue
        t.attempt((shape, "sw_stats_cross"), adm, lambda: grid(ctx.sw_stats_cross(q, tg, sc)), same(wanted), "sw_stats_cross")
        t.attempt((shape, "sw_span_cross"), adm, lambda: grid(ctx.sw_span_cross(q, tg, sc)), same([[x[:5] for x in row] for row in wanted]),
                  "sw_span_cross")
        for min_score in (1, thr(cs[0])):
            def search():
                n_hits, hits = ctx.sw_span_search(q, tg, sc, 3, min_score=min_score)
                assert hits.dtype == S.SPAN_HIT and hits.shape == (n, 3)
                return [[tuple(int(h[f]) for f in ("target", "score", "pos_a", "pos_b", "len_a", "len_b")) for h in hits[i, :int(n_hits[i])]]
                        for i in range(n)]
            t.attempt((shape, "sw_span_search", min_score), adm, search, same(top_k(wanted, 3, min_score)), "sw_span_search")
    FAMILIES_RUN.add(("sets", fam))
    t.done(G.family_id(fam))


# ------------------------------------------------------------------------------- H. the banded statistics and span calls ---
SPAN_BAND_MAX_WIDTH = 512       # SEQALIGN_SPAN_BAND_MAX_WIDTH: the narrow statistics and span calls' cap


def traceback_or(fn):
    """fn's result, or the message of its SEQALIGN_E_TRACEBACK; any other error passes through."""
    def call():
        try:
            return fn()
        except S.SeqAlignError as e:
            if e.code != S.E_TRACEBACK:
                raise
            return str(e)
    return call


def same_bytes(narrow, wide):
    """Two calls' results array by array, byte for byte -- or both raise the same code."""
    out = []
    for fn in (narrow, wide):
        try:
            out.append(b"".join(x.tobytes() for x in fn()))
        except S.SeqAlignError as e:
            out.append(e.code)
    return out[0] == out[1], [x if isinstance(x, int) else len(x) for x in out]


@FAMS
def test_banded_stats_and_span_calls(ctx, fam):
    """nw_stats_banded, sw_stats_banded and the three wide forms at strips of 64 columns, under test_banded_calls' three bands
    per pair.  NW: bandlib.expected_both's end value and the counted strings of the oracle's walk over the banded matrices;
    where that walk fails the call returns SEQALIGN_E_TRACEBACK naming the lowest such pair, and the group runs again without
    those pairs.  SW: the banded hit at min_score = 1 and its counted strings.  The narrow calls take at most 512 diagonals and
    run where the group's widths allow; there narrow and wide agree on bytes and on status.
    Under the deep families the banded end values of the long shapes stand below INT32_MIN / 2 and the oracle still walks
    them: the value alone does not tell whether a pair has an alignment inside its band."""
    t = Tally()
    deep = 0
    for shape, is_sw, cs, batch, sc, la, lb in group_of(fam):
        adm = G.admitted(cs[0].spec, la, lb, "band")
        for k in range(3):
            if is_sw:
                n = len(cs)
                lo, hi = (np.array(v, np.int32) for v in zip(*[sw_band_of(c, k) for c in cs]))
                w7 = [want("sw_band_stats", c, *sw_band_of(c, k)) for c in cs]
                narrow = max(BS.width_of(len(c.a), len(c.b), *sw_band_of(c, k)) for c in cs) <= SPAN_BAND_MAX_WIDTH
                with ctx.options(band_strip_cols=STRIP):
                    t.attempt((shape, k, "sw_stats_banded_wide"), adm, lambda: rows_of(ctx.sw_stats_banded_wide(batch, sc, lo, hi), n),
                              lambda g: first_diff(g, w7), "sw_stats_banded_wide")
                    t.attempt((shape, k, "sw_span_banded_wide"), adm, lambda: rows_of(ctx.sw_span_banded_wide(batch, sc, lo, hi), n),
                              lambda g: first_diff(g, [x[:5] for x in w7]), "sw_span_banded_wide")
                    if narrow:
                        t.attempt((shape, k, "sw_stats_banded"), adm, lambda: rows_of(ctx.sw_stats_banded(batch, sc, lo, hi), n),
                                  lambda g: first_diff(g, w7), "sw_stats_banded")
                        for a_, b_ in ((ctx.sw_stats_banded, ctx.sw_stats_banded_wide), (ctx.sw_span_banded, ctx.sw_span_banded_wide)):
                            ok, what = same_bytes(lambda: a_(batch, sc, lo, hi), lambda: b_(batch, sc, lo, hi))
                            assert ok, (shape, k, a_.__name__, what)
                continue
            bands = [nw_band_of(c, k) for c in cs]
            both = [want("nw_band_stats", c, w) for c, w in zip(cs, bands)]
            calls = [("nw_stats_banded_wide", ctx.nw_stats_banded_wide)]
            if max(BL.width_of(len(c.a), len(c.b), w) for c, w in zip(cs, bands)) <= SPAN_BAND_MAX_WIDTH:
                calls.append(("nw_stats_banded", ctx.nw_stats_banded))
            none = [p for p, x in enumerate(both) if x[1] is None]
            keep = [p for p in range(len(cs)) if p not in none]
            kept = W.from_pairs([(cs[p].a, cs[p].b) for p in keep]) if none and keep else batch
            bw, bw_kept = np.array(bands, np.uint32), np.array([bands[p] for p in keep], np.uint32)
            wanted = [both[p][1] for p in keep]
            with ctx.options(band_strip_cols=STRIP):
                for name, fn in calls:
                    if none:        # no alignment inside the band: the call says so and names the lowest such pair
                        t.attempt((shape, k, name, "none"), adm, traceback_or(lambda: fn(batch, sc, bw)),
                                  lambda g: None if isinstance(g, str) and f"pair {none[0]}:" in g else f"pairs {none} have no walk: got {g}")
                    if keep:
                        before = t.exact
                        t.attempt((shape, k, name), adm, lambda: rows_of(fn(kept, sc, bw_kept), len(keep)),
                                  lambda g: first_diff(g, wanted), name)
                        deep += (t.exact > before) * sum(x[0] < -2 ** 30 for x in wanted)
                if len(calls) == 2:
                    ok, what = same_bytes(lambda: calls[1][1](batch, sc, bw), lambda: calls[0][1](batch, sc, bw))
                    assert ok, (shape, k, what)
                    if none and keep:
                        ok, what = same_bytes(lambda: calls[1][1](kept, sc, bw_kept), lambda: calls[0][1](kept, sc, bw_kept))
                        assert ok, (shape, k, what)
    print(f"{G.family_id(fam)}: {deep} banded NW statistics below -2^30 equal to the oracle's walk")
    FAMILIES_RUN.add(("banded", fam))
    t.done(G.family_id(fam))
    if fam[1] == G.DEEP:
        assert deep > 0, "no banded statistics result below -2^30 from a deep family"


def test_every_new_call_met_both_sides():
    """Over the whole matrix each of the eleven calls of sections G and H returned the oracle's answer at least once and was
    refused with SEQALIGN_E_DOMAIN at least once (tests/test_magnitude_argument_cpu.py argues on the CPU that the matrix holds
    such groups).  Counted over the tests of sections G and H; where not all of them ran before this one in the same process
    (a selection, another order, several workers) there is nothing to assert and the test skips."""
    print({name: tuple(CALL_COUNTS.get(name, (0, 0))) for name in NEW_CALLS})
    missing = {(sec, f) for sec in ("stats", "sets", "banded") for f in G.FAMILIES} - FAMILIES_RUN
    if missing:
        pytest.skip(f"{len(missing)} (section, family) tests of sections G and H did not run before this one in this process")
    for name in NEW_CALLS:
        exact, refused = CALL_COUNTS.get(name, (0, 0))
        assert exact > 0 and refused > 0, (name, exact, refused)
