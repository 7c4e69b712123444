"""GPU tier: gap-dense alignments through every direction fill and every walker.

The direction-byte paths (sa_fill_dirs.hip, sa_fill_dirs_x2.hip, sa_fill_nw_dirs_x1.hpp, the walkers of sa_traceback.hip, the
sweep of sa_sw_sweep.hip, the plane decoders of host/sa_moves.c) never write the three matrices: a wrong bit in a direction byte
shows only through a walk that reads it.  Under the two scorings nearly every other GPU test uses no optimal alignment puts an
insertion run directly against a deletion run, so no walk ever stands in GAP_A with a GAP_B predecessor (SA_LD_BM through
local_depart; the TY fallback of the older byte).  Here every pair has such transitions -- tests/test_dense_argument_cpu.py
counts them, pair by pair, on the oracle alone -- on every position of a move word, a tile edge and a direction block
(tests/denselib.py), with CIGARs longer than the gapped strings, and under a scoring where every comparison ties.

Every result is compared with the oracle (needleman_wunsch.c:34-146, smith_waterman.c:137-277): score, both strings, hit lists,
CIGAR bytes; every case asks the library what it launched (seqalign_ctx_last_call_info), so that none passes on another path.
"""
import pytest

import denselib as D
import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu
M, EQX = D.M, D.EQX
THR = D.SW_MIN_SCORE


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


@pytest.fixture
def opts(ctx):
    changed = {}

    def set_(**kv):
        for k, v in kv.items():
            changed.setdefault(k, ctx.get_option(k))
            ctx.set_option(k, v)
    yield set_
    for k, v in changed.items():
        ctx.set_option(k, v)


_SC, _NW, _SW = {}, {}, {}


def scoring(name):
    if name not in _SC:
        _SC[name] = S.make_scoring(D.SCORINGS[name])
    return _SC[name]


def want_nw(name, a, b):
    """The oracle's global alignment, computed once per pair and scoring for the whole file."""
    key = (name, a, b)
    if key not in _NW:
        rc, s, ra, rb = O.oracle_nw(D.oracle_scoring(name), a, b)
        assert rc == 0
        _NW[key] = (s, ra, rb)
    return _NW[key]


def want_sw(name, a, b, max_hits):
    """The oracle's hit list at min_score THR: all of it once, a prefix per call (hits come out in the reference's order)."""
    key = (name, a, b)
    have = _SW.get(key)
    if have is None or (max_hits > have[0] and len(have[1]) == have[0]):      # nothing yet, or a list cut short of what is asked now
        rc, hits = O.oracle_sw(D.oracle_scoring(name), a, b, THR, max_hits)
        assert rc == 0
        have = _SW[key] = (max_hits, hits)
    return have[1][:max_hits]


def singles(pairs):
    """How many pairs of a ragged chunk find no partner of their shape (they get a wave to themselves)."""
    shapes = {}
    for a, b in pairs:
        shapes[(len(a), len(b))] = shapes.get((len(a), len(b)), 0) + 1
    return sum(v % 2 for v in shapes.values())


def check_nw(ctx, name, pairs, label):
    got = ctx.nw_batch(W.from_pairs(pairs), scoring(name))
    ran = ctx.last_call()
    for p, (a, b) in enumerate(pairs):
        assert got[p] == want_nw(name, a, b), (label, name, p, len(a), len(b), ran)
    return ran


def check_sw(ctx, name, pairs, max_hits, label):
    got = ctx.sw_batch(W.from_pairs(pairs), scoring(name), THR, max_hits=max_hits, hit_cap=1 << 16)
    ran = ctx.last_call()
    for p, (a, b) in enumerate(pairs):
        assert got[p] == want_sw(name, a, b, max_hits), (label, name, max_hits, p, len(a), len(b), ran)
    return ran


def fills_of(ran):
    return {k: v[1] for k, v in ran.items() if k.startswith("fill_")}


# ------------------------------------------------------------------ NW: the six scorings x the four forms of the fill ---

@pytest.mark.parametrize("form", ["x1", "x2", "x4", "mixed"])
@pytest.mark.parametrize("name", D.NW_SCORINGS)
def test_nw_dense_through_every_fill(ctx, opts, name, form):
    """seqalign_nw_batch on alternation and spaced pairs at 150 x 150, 31 x 40, 191 x 150, m = 250 (8 columns per lane), m = 500 and
    the short-b wide form (16 per lane): one pair per wave, two per wave (one shape, and ragged with partners found by shape),
    four per wave (rows <= 192 columns), and a mostly-one-shape batch that launches both kinds of waves in one grid."""
    for shape in (D.QUAD_SHAPES if form == "x4" else D.NW_SHAPES):
        uni, rag, extra = D.nw_uniform(shape, name), D.nw_ragged(shape, name), D.nw_extra(shape, name)
        if form == "x1":
            opts(pack16=0)
            pairs = (uni if len(uni) < 100 else []) + rag + extra
            ran = check_nw(ctx, name, pairs, (form, shape))
            assert fills_of(ran) == {"fill_nw_dirs": len(pairs)} and ran["walk_moves_tile"] == (1, len(pairs)), (shape, ran)
        elif form == "x2":
            opts(pack16=2, quad=1)
            ran = check_nw(ctx, name, uni, (form, shape))
            assert fills_of(ran) == {"fill_nw_dirs_x2": len(uni)} and ran["walk_moves_tile"] == (1, len(uni)), (shape, ran)
            pairs = rag + extra
            ran = check_nw(ctx, name, pairs, (form, shape, "ragged"))
            alone = singles(pairs)
            assert alone and fills_of(ran) == {"fill_nw_dirs_x2": len(pairs) - alone, "fill_nw_dirs": alone}, (shape, ran)
        elif form == "x4":
            opts(pack16=2, quad=2)
            pairs = uni + [p for p in extra if (len(p[0]), len(p[1])) == (len(uni[0][0]), len(uni[0][1]))]
            ran = check_nw(ctx, name, pairs, (form, shape))
            assert fills_of(ran) == {"fill_nw_dirs_x4": len(pairs)} and ran["walk_moves_tile"] == (1, len(pairs)), (shape, ran)
        else:
            opts(pack16=2)
            pairs = D.nw_mostly_one_shape(shape, name)
            ran = check_nw(ctx, name, pairs, (form, shape))
            alone = singles(pairs)
            assert alone >= 2 and fills_of(ran) == {"fill_nw_dirs_x2": len(pairs) - alone, "fill_nw_dirs": alone}, (shape, ran)


# ------------------------------------------------------------------ NW: the walkers and the rest, one axis at a time ---

# (options, the kernels the call must launch) -- one parameter away from the default each
NW_AXES = {
    "default": ({}, {"fill_nw_dirs", "walk_moves_tile"}),
    "dirs_local=0": (dict(dirs_local=0), {"fill_nw_dirs", "walk_moves_tile"}),
    "lane": (dict(trace_kernel="lane"), {"fill_nw_dirs", "walk_moves_lane"}),
    "wave": (dict(trace_kernel="wave"), {"fill_nw_dirs", "walk_moves_tile"}),
    "walk_group=1": (dict(walk_group=1), {"fill_nw_dirs", "walk_moves_tile"}),
    "walk_group=4": (dict(walk_group=4), {"fill_nw_dirs", "walk_moves_tile"}),
    "walk_group=8": (dict(walk_group=8), {"fill_nw_dirs", "walk_moves_tile"}),
    "walk_tile=32": (dict(walk_tile=32), {"fill_nw_dirs", "walk_moves_tile"}),
    "walk_tile=64": (dict(walk_tile=64), {"fill_nw_dirs", "walk_moves_tile"}),
    "walk_stage=0": (dict(walk_tile=64, walk_stage=0), {"fill_nw_dirs", "walk_moves_tile"}),
    "nw_moves=0": (dict(nw_moves=0), {"fill_nw_dirs", "walk_dirs_tile"}),
    "nw_moves=0,lane": (dict(nw_moves=0, trace_kernel="lane"), {"fill_nw_dirs", "walk_dirs_lane"}),
    "host": (dict(traceback="host"), None),
    "nw_dirs=0": (dict(nw_dirs=0), {"fill_stream", "walk_wave"}),
    "subbatches=3": (dict(subbatches=3), {"fill_nw_dirs", "walk_moves_tile"}),
}


@pytest.mark.parametrize("axis", list(NW_AXES))
def test_nw_dense_through_every_walker(ctx, opts, axis):
    """150 x 150 and m = 250 under [2,-9,0,-1] and [1,0,0,0], ragged batches of alternation, spaced and substituted pairs: both
    forms of the byte, the lane and the tile walkers, one / four / eight walks per wave, both tile edges, moves leaving in one run
    or in two pieces, strings instead of moves, the host traceback, the three matrices, sub-batches."""
    kv, kernels = NW_AXES[axis]
    opts(**kv)
    for name in ("cheap0", "ties"):
        for shape in ("150x150", "m250"):
            pairs = D.walker_pairs(shape, name) + D.nw_extra(shape, name)
            ran = check_nw(ctx, name, pairs, (axis, shape))
            if kernels is None:
                assert not any(k.startswith("walk_") for k in ran), (axis, ran)      # the walk was the host's
            else:
                assert set(ran) == kernels, (axis, shape, ran)
                walk = [k for k in kernels if k.startswith("walk_")][0]
                assert ran[walk][1] == len(pairs) and (axis == "subbatches=3") == (ran["fill_nw_dirs" if "fill_nw_dirs" in ran else "fill_stream"][0] > 1), (axis, ran)


WALKER_KINDS = {
    "tile-local": {},
    "tile-local-32": dict(walk_tile=32),
    "tile-older-byte": dict(dirs_local=0, trace_kernel="wave"),
    "tile-group-4": dict(walk_group=4),
    "lane": dict(trace_kernel="lane"),
    "strings-tile": dict(nw_moves=0),
    "three-matrices": dict(nw_dirs=0),
    "host": dict(traceback="host"),
}


@pytest.mark.parametrize("kind", list(WALKER_KINDS))
def test_long_runs_and_staircases_once_per_walker(ctx, opts, kind):
    """An insertion run and a deletion run of ~200 columns back to back (the transition at the end of runs that cross several
    tiles in a gap state), and disjoint alphabets (len_a I, then len_b D, nothing else): one pair per wave and two."""
    opts(**WALKER_KINDS[kind])
    pairs = D.long_run_pairs()
    for name in ("cheap0", "ties", "ext0"):
        for pack in (0, 2):
            opts(pack16=pack)
            ran = check_nw(ctx, name, pairs, (kind, pack))
            if kind not in ("three-matrices", "host"):
                assert any(k.startswith("fill_nw_dirs") for k in ran) and ("fill_nw_dirs_x2" in ran) == (pack == 2), (kind, ran)


# ------------------------------------------------------------------ SW best hit ---

@pytest.mark.parametrize("form", ["x2", "x4", "unpacked", "three-matrices", "older-byte", "lane", "tile-32", "tile-64", "strings"])
@pytest.mark.parametrize("name", D.SW_SCORINGS)
def test_sw_best_hit_dense(ctx, opts, name, form):
    """seqalign_sw_batch(max_hits = 1): the packed best-hit fills two and four per wave (one shape), their one-pair form (ragged:
    partners by shape, a pair without one has a wave to itself -- the best-hit call has no other one-pair direction fill), the
    call without packing and with the direction bytes switched off (three matrices either way), the older byte, the lane walker,
    both tile edges, strings instead of moves -- the best hit of an alternation pair is the whole pair, every period walked."""
    kv = {"x2": dict(pack16=2, quad=1), "x4": dict(pack16=2, quad=2), "unpacked": dict(pack16=0), "three-matrices": dict(pack16=2, sweep_dirs=0, nw_dirs=0),
          "older-byte": dict(pack16=2, dirs_local=0), "lane": dict(pack16=2, trace_kernel="lane"), "tile-32": dict(pack16=2, walk_tile=32),
          "tile-64": dict(pack16=2, walk_tile=64, walk_stage=0), "strings": dict(pack16=2, nw_moves=0)}[form]
    opts(**kv)
    walk = {"lane": "walk_moves_lane", "strings": "walk_dirs_tile"}.get(form, "walk_moves_tile")
    for shape in (D.QUAD_SHAPES if form == "x4" else D.SW_SHAPES):
        uni, rag = D.sw_uniform(shape, name), D.sw_ragged(shape, name)
        ran = check_sw(ctx, name, uni, 1, (form, shape))
        if form == "x4":
            assert ran == {"fill_sw_best_x4": (1, len(uni)), walk: (1, len(uni))}, (shape, ran)
        elif form in ("unpacked", "three-matrices"):
            assert ran == {"fill_stream": (1, len(uni)), "walk_wave": (1, len(uni))}, (shape, ran)
        else:
            assert ran == {"fill_sw_best_x2": (1, len(uni)), walk: (1, len(uni))}, (shape, ran)
        ran = check_sw(ctx, name, rag, 1, (form, shape, "ragged"))
        if form in ("unpacked", "three-matrices"):
            assert ran == {"fill_stream": (1, len(rag)), "walk_wave": (1, len(rag))}, (shape, ran)
        else:       # (a pair list: two per wave whatever `quad` says; a wave's two slots are counted, filled or not)
            alone = singles(rag)
            assert alone and ran == {"fill_sw_best_x2": (1, len(rag) + alone), walk: (1, len(rag))}, (shape, ran)


# ------------------------------------------------------------------ SW multi-hit ---

MULTI = {
    "pack16=0": (dict(pack16=0), {"fill_sw_dirs", "sweep_dirs"}),
    "pack16=2": (dict(pack16=2), {"fill_sw_dirs_x2", "sweep_dirs"}),
    "sweep_ev=0": (dict(sweep_ev=0), {"fill_sw_dirs", "sweep_dirs"}),
    "sweep_ev=0,pack16=2": (dict(sweep_ev=0, pack16=2), {"fill_sw_dirs_x2", "sweep_dirs"}),
    "pair": (dict(sweep_mode="pair"), {"fill_sw_dirs", "sweep_dirs"}),
    "strips": (dict(sweep_mode="strips"), {"sweep_strips"}),
    "sweep_dirs=0": (dict(sweep_dirs=0), {"fill_stream", "sweep_regs"}),
}


@pytest.mark.parametrize("config", list(MULTI))
@pytest.mark.parametrize("name", D.SW_SCORINGS)
def test_sw_multi_hit_dense(ctx, opts, name, config):
    """max_hits 4 (the one-trip call) and unlimited (three trips), min_score 4: one pair per wave and two, both sweep forms on
    direction bytes, the pair and the strip sweep, the three matrices.  Spaced alternation with the stretch planted twice: several
    dense hits share cells, and the visited mask cuts a walk inside an 1I1D."""
    kv, kernels = MULTI[config]
    opts(**kv)
    for label, pairs in (("150x150", D.sw_uniform("150x150", name)), ("31x40", D.sw_uniform("31x40", name)),
                         ("191x150 ragged", D.sw_ragged("191x150", name)), ("planted twice", D.sw_planted_twice(name))):
        for max_hits in (4, 1 << 20):
            ran = check_sw(ctx, name, pairs, max_hits, (config, label))
            assert kernels <= set(ran), (config, label, max_hits, ran)
            if "fill_sw_dirs" in kernels:
                assert "fill_sw_dirs_x2" not in ran and "fill_stream" not in ran, (config, label, ran)
            if config == "sweep_dirs=0":
                assert not any("dirs" in k for k in ran), (config, label, ran)


# ------------------------------------------------------------------ the CIGAR calls ---

@pytest.mark.parametrize("where", ["device", "device-three-matrices", "host"])
def test_nw_cigar_longer_than_the_strings(ctx, opts, where):
    """seqalign_nw_batch_cigar on the alternation pairs, both formats: 1M1I1D per period -- 450 bytes where the strings' slot is 301.
    The default (worst-case) slots deliver denselib's CIGAR of the oracle's strings, a slot of len + 1 does, a slot of len is
    SEQALIGN_E_NOMEM as the header documents; from the planes, from the three matrices' strings and from the host traceback."""
    if where == "device-three-matrices":
        opts(nw_dirs=0)
    elif where == "host":
        opts(traceback="host")
    for name, shape in (("cheap0", "150x150"), ("ties", "150x150"), ("ext0", "191x150"), ("cheap0N", "m250")):
        pairs = D.nw_uniform(shape, name)
        batch = W.from_pairs(pairs)
        for fmt in (M, EQX):
            want = [(want_nw(name, a, b)[0], D.cigar(*want_nw(name, a, b)[1:], fmt).encode()) for a, b in pairs]
            got = ctx.nw_batch_cigar(batch, scoring(name), fmt)
            ran = ctx.last_call()
            if where == "device":
                assert set(ran) == {"fill_nw_dirs", "walk_moves_tile"}, ran
            elif where == "device-three-matrices":
                assert set(ran) == {"fill_stream", "walk_wave"}, ran
            assert got == want, (where, name, fmt)
            longest = max(len(c) for _, c in want)
            if D.matches_of(name) == 1:
                assert longest > len(pairs[0][0]) + len(pairs[0][1]) + 1
            off, out, out_len, out_score = ctx.nw_batch_cigar(batch, scoring(name), fmt, slot=longest + 1, raw=True)
            for p, (s, c) in enumerate(want):
                assert out[int(off[p]):int(off[p]) + int(out_len[p]) + 1].tobytes() == c + b"\0" and out_score[p] == s, (where, name, fmt, p)
            with pytest.raises(S.SeqAlignError) as e:
                ctx.nw_batch_cigar(batch, scoring(name), fmt, slot=longest)
            assert e.value.code == S.E_NOMEM


@pytest.mark.parametrize("where", ["device", "device-three-matrices", "host"])
def test_sw_cigar_longer_than_the_strings(ctx, opts, where):
    """seqalign_sw_batch_cigar on the alternation pairs: the best hit of (AC)^75 x (AG)^75 has 223 columns and a 446-byte CIGAR.
    max_hits 1 (planes from the packed best-hit call), 4 (planes, one trip) and unlimited (strings); a buffer that holds all CIGARs
    back to back exactly is enough, one byte less is SEQALIGN_E_NOMEM."""
    if where == "device-three-matrices":
        opts(sweep_dirs=0, nw_dirs=0)
    elif where == "host":
        opts(traceback="host")
    for name in D.SW_SCORINGS:
        pairs = D.sw_uniform("150x150", name)[:15] + [(b"AC" * 75, b"AG" * 75)]
        batch = W.from_pairs(pairs)
        for max_hits, fmt, pack in ((1, M, 2), (1, EQX, 0), (4, EQX, 2), (4, M, 0), (1 << 20, M, 1)):
            opts(pack16=pack)
            want = [[dict(score=h["score"], pos_a=h["pos_a"], pos_b=h["pos_b"], len_a=h["len_a"], len_b=h["len_b"], length=len(h["a"]),
                          cigar=D.cigar(h["a"], h["b"], fmt)) for h in want_sw(name, a, b, max_hits)] for a, b in pairs]
            got = ctx.sw_batch_cigar(batch, scoring(name), THR, max_hits=max_hits, fmt=fmt, hit_cap=1 << 16, cigar_cap=1 << 22)
            ran = ctx.last_call()
            assert got == want, (where, name, max_hits, fmt)
            if where == "device" and max_hits == 1 and pack == 2:
                assert "fill_sw_best_x2" in ran and "walk_moves_tile" in ran, ran
            if where == "device" and max_hits == 4:
                assert ("fill_sw_dirs_x2" if pack else "fill_sw_dirs") in ran and "walk_moves_tile" in ran, ran
            if name != "ext0":
                assert len(want[-1][0]["cigar"]) == 446 and want[-1][0]["length"] == 223
            used = sum(len(h["cigar"]) + 1 for hits in want for h in hits)
            n_hits = sum(len(hits) for hits in want)
            rc, n, _, _ = ctx.sw_batch_cigar(batch, scoring(name), THR, max_hits=max_hits, fmt=fmt, hit_cap=1 << 16, cigar_cap=used, raw=True)
            assert (rc, n) == (0, n_hits), (where, name, max_hits, fmt, used)
            rc, n, _, _ = ctx.sw_batch_cigar(batch, scoring(name), THR, max_hits=max_hits, fmt=fmt, hit_cap=1 << 16, cigar_cap=used - 1, raw=True)
            assert rc == S.E_NOMEM and n < n_hits, (where, name, max_hits, fmt, used)


# ------------------------------------------------------------------ the neighbouring calls ---

@pytest.mark.parametrize("rows", [7, 64])
def test_nw_align_long_seams_inside_alternating_stretches(ctx, opts, rows):
    """seqalign_nw_align_long with blocks of 7 and 64 rows: with a period of two rows per 1I1D every block seam falls inside an
    alternating stretch (7 is odd: on either row of the period in turn)."""
    opts(long_block_rows=rows)
    pairs = [D.alternation(150, 150, 0), D.alternation(191, 150, 4), D.alternation(500, 500, 1), D.spaced(300, 260, 11, 2),
             D.spaced(150, 150, 12, 3), D.alternation(31, 40, 5)] + D.long_run_pairs()[:2]
    got = ctx.nw_align_long(W.from_pairs(pairs), scoring("cheap0"))
    ran = ctx.last_call()
    assert {"long_forward", "long_block", "long_walk"} <= set(ran), ran
    for p, (a, b) in enumerate(pairs):
        assert got[p] == want_nw("cheap0", a, b), (rows, p)


def test_nw_align_banded_holds_the_alternation(ctx):
    """seqalign_nw_align_banded, band 3: the alternation's diagonal excursion is 1, so the banded result is seqalign_nw_batch's byte
    for byte."""
    import bandlib as B
    pairs = [D.alternation(150, 150, k) for k in range(12)] + [D.alternation(500, 500, 2), D.spaced(150, 150, 12, 3)]
    for a, b in pairs:
        s, ra, rb = want_nw("cheap0", a, b)
        assert B.excursion(ra, rb) in ((-1, 0), (0, 1), (-1, 1)) and D.count_id(ra, rb) >= 8
    batch = W.from_pairs(pairs)
    got = ctx.nw_align_banded(batch, scoring("cheap0"), 3)
    ran = ctx.last_call()
    assert {"band_fill", "band_walk"} <= set(ran), ran
    assert got == ctx.nw_batch(batch, scoring("cheap0")) == [want_nw("cheap0", a, b) for a, b in pairs]
