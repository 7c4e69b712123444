"""GPU tier: alignments of pairs of any size -- seqalign_nw_align_long / seqalign_sw_align_long (sa_align_long.hip,
sa_batch_long.hip).

The calls must return what seqalign_nw_batch and seqalign_sw_batch(max_hits = 1) return, byte for byte, for every pair those
accept -- checked here on small pairs with forced block heights (option long_block_rows) so that the checkpoint / block /
walk hand-offs run many times, against the existing calls and the oracle -- and must align pairs past the 2^31-cell cap.
"""
import itertools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
ROWS = [1, 3, 64, 0]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def oracle_scoring_of(sc):
    return O.Scoring.from_buffer_copy(bytes(sc))


def check_nw(ctx, batch, sc, tag=""):
    want = ctx.nw_batch(batch, sc)
    got = ctx.nw_align_long(batch, sc)
    bad = [(p, got[p], want[p]) for p in range(batch.n_pairs) if got[p] != want[p]]
    assert not bad, (tag, bad[:3])
    assert set(ctx.last_call()) <= {"long_forward", "long_block", "long_walk"}, ctx.last_call()
    return got


def check_sw(ctx, batch, sc, min_score, tag=""):
    want = ctx.sw_batch(batch, sc, min_score, max_hits=1)
    got = ctx.sw_align_long(batch, sc, min_score)
    bad = [(p, got[p], want[p]) for p in range(batch.n_pairs) if got[p] != want[p]]
    assert not bad, (tag, bad[:3])
    assert set(ctx.last_call()) <= {"long_forward", "long_block", "long_walk"}, ctx.last_call()
    return got


def check_oracle(batch, sc, got_nw, got_sw, min_score, pairs):
    osc = oracle_scoring_of(sc)
    for p in pairs:
        a, b = batch.seq_a(p), batch.seq_b(p)
        if got_nw is not None:
            rc, score, ra, rb = O.oracle_nw(osc, a, b)
            assert rc == 0 and got_nw[p] == (score, ra, rb), (p, got_nw[p], (score, ra, rb))
        if got_sw is not None:
            rc, hits = O.oracle_sw(osc, a, b, min_score, 1)
            assert rc == 0 and got_sw[p] == hits[:1], (p, got_sw[p], hits[:1])


def related(rng, n, alpha, edits=0.1):
    """A random sequence and a copy with about `edits` of its positions substituted, deleted or followed by an insertion."""
    al = np.frombuffer(alpha, np.uint8)
    a = al[rng.below(len(al), n).astype(np.int64)]
    kind = rng.below(100, n).astype(np.int64)
    subs = al[rng.below(len(al), n).astype(np.int64)]
    cut = int(edits * 100)
    out = []
    for i in range(n):
        k = kind[i]
        if k < cut // 3:
            out.append(int(subs[i]))
        elif k < 2 * cut // 3:
            continue
        elif k < cut:
            out.append(int(a[i])); out.append(int(subs[i]))
        else:
            out.append(int(a[i]))
    return a.tobytes(), bytes(out)


EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1400]


def edge_batch(seed, alpha):
    """Ragged pairs whose lengths cross the strip (512) and one-wave (1 024) widths on both sides; half of them related."""
    rng = W.Rng(seed)
    pairs = []
    for k, la in enumerate(EDGE_LENGTHS):
        lb = EDGE_LENGTHS[(5 * k + 3) % len(EDGE_LENGTHS)]
        if k % 2:
            a, b = related(rng, max(la, lb), alpha)
            pairs.append((a[:la], b[:lb]))
        else:
            al = np.frombuffer(alpha, np.uint8)
            pairs.append((al[rng.below(len(al), la).astype(np.int64)].tobytes(),
                          al[rng.below(len(al), lb).astype(np.int64)].tobytes()))
    return W.from_pairs(pairs)


# ---------------------------------------------------------------- 1. small pairs, every flag --
@pytest.mark.parametrize("rows", ROWS)
def test_golden_cases_equal_the_existing_calls(ctx, rows):
    """Every case of fill_small.json (the compiled reference's inputs, all flag combinations): nw_batch's and best-hit
    sw_batch's bytes, with blocks of `rows` rows; the golden NW strings where recorded."""
    n = 0
    with ctx.options(long_block_rows=rows):
        for case in json.loads((GOLD / "fill_small.json").read_text())["cases"]:
            sc = S.make_scoring(case["scoring"])
            batch = W.from_pairs([(g["a"].encode(), g["b"].encode()) for g in case["pairs"]])
            got = check_nw(ctx, batch, sc, case["scoring"])
            for p, g in enumerate(case["pairs"]):
                if "result_a" in g["nw"]:
                    assert got[p] == (g["nw"]["score"], g["nw"]["result_a"].encode(), g["nw"]["result_b"].encode())
            check_sw(ctx, batch, sc, 3, case["scoring"])
            n += batch.n_pairs
    assert n >= 100


@pytest.mark.parametrize("rows", [3, 0])
def test_all_flag_combinations(ctx, rows):
    """The 32 combinations of the reference's five flags (the GENERAL row sweep), wildcards and mutations, ragged pairs."""
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        sc = S.make_scoring(spec)
        batch = W.ragged(12, seed=900 + idx, max_len=90, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        with ctx.options(long_block_rows=rows):
            nw = check_nw(ctx, batch, sc, flags)
            sw = check_sw(ctx, batch, sc, 2, flags)
        if idx % 4 == 0:
            check_oracle(batch, sc, nw, sw, 2, range(0, 12, 3))


SCORINGS = {
    "dna": ({"preset": "default"}, b"ACGT"),
    "dna_open_pos": ({"init": [2, -3, 1, -2, 0, 0, 0, 0, 0, 0]}, b"ACGT"),     # gap_open > 0: the GENERAL path
    "blosum62": ({"preset": "BLOSUM62"}, b"ARNDCQEGHILKMFPSTWYV"),
}


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", list(SCORINGS))
def test_ragged_widths_across_strip_edges(ctx, name, rows):
    """Lengths 0 .. 1 400 across 511 / 512 / 513 and 1 024 / 1 025: nw_batch, best-hit sw_batch with a min_score that
    filters some pairs out, and the oracle on a sample."""
    spec, alpha = SCORINGS[name]
    sc = S.make_scoring(spec)
    batch = edge_batch(4000 + len(name), alpha)
    with ctx.options(long_block_rows=rows):
        nw = check_nw(ctx, batch, sc, (name, rows))
        sw = check_sw(ctx, batch, sc, 40, (name, rows))
    assert any(not h for h in sw) and any(h for h in sw)
    if rows in (3, 0):
        check_oracle(batch, sc, nw, sw, 40, [1, 5, 8, 11])


# ---------------------------------------------------------------- 2. block edges --
def edge_pairs(rng):
    al = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda n: al[rng.below(4, n).astype(np.int64)].tobytes()
    x, y, g = rnd(70), rnd(60), rnd(45)
    run = rnd(200)
    pre = rnd(100)
    return [
        (x + y, x + g + y),          # a long gap in a (gap_b run across block rows)
        (x + g + y, x + y),          # a long gap in b
        (run, run),                  # one match run over every checkpoint row
        (run[:150], run[20:]),       # ... off the diagonal
        (pre + x, x),                # the walk reaches row 0 inside a block; NW: leading gaps in b
        (x, pre + x),                # ... column 0; NW: leading gaps in a
        (rnd(33), rnd(97)),
    ]


@pytest.mark.parametrize("rows", [16, 17])
@pytest.mark.parametrize("spec", [{"preset": "default"}, {"init": [1, -2, -4, -1, 1, 1, 0, 0, 0, 0]},
                                  {"init": [2, -2, -3, -1, 0, 0, 0, 0, 0, 0]}])
def test_block_edges(ctx, rows, spec):
    """Constructed pairs whose walks cross checkpoint rows in a gap of a, a gap of b and a run of matches, and reach row 0 /
    column 0 inside a block: the existing calls' bytes, the oracle's, and several blocks per pair."""
    sc = S.make_scoring(spec)
    batch = W.from_pairs(edge_pairs(W.Rng(31 + rows)))
    with ctx.options(long_block_rows=rows):
        nw = check_nw(ctx, batch, sc, (spec, rows))
        blocks = ctx.last_call()["long_block"][0]
        sw = check_sw(ctx, batch, sc, 1, (spec, rows))
    assert blocks > 2 * batch.n_pairs, blocks
    if "preset" in spec:   # default scoring, no free end gaps: the NW leading gaps are there
        assert nw[4][2].startswith(b"-" * 100) and nw[5][1].startswith(b"-" * 100), (nw[4], nw[5])
    check_oracle(batch, sc, nw, sw, 1, range(batch.n_pairs))


# ---------------------------------------------------------------- 3. wide rows --
@pytest.mark.parametrize("name", ["dna", "blosum62"])
def test_wide_rows_general_flags(ctx, name):
    """3 000 x 2 500 pairs (6 strips per row) with free end gaps and R = 100: nw_batch and the oracle."""
    spec, alpha = SCORINGS[name]
    spec = dict(spec)
    spec["flags"] = {"no_start_gap_penalty": 1, "no_end_gap_penalty": 1}
    sc = S.make_scoring(spec)
    rng = W.Rng(77 + len(name))
    a, b = related(rng, 3000, alpha, 0.15)
    batch = W.from_pairs([(a, b[:2500]), (a[400:2900], a)])
    with ctx.options(long_block_rows=100):
        nw = check_nw(ctx, batch, sc, name)
        assert ctx.last_call()["long_block"][0] >= 40
        sw = check_sw(ctx, batch, sc, 50, name)
    check_oracle(batch, sc, nw, sw, 50, [0, 1])


# ---------------------------------------------------------------- 4. beyond the cap --
BEYOND_CAP = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[1] + "/seq-align_amd/python", sys.argv[1] + "/tests"]
import seqalign_amd as S
from seqalign_amd import workloads as W
from test_gpu_align_long import related, rescore

which = sys.argv[2]
rng = W.Rng(60000)
with S.Context(0) as ctx:
    nw = S.make_scoring({"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]})
    sw = S.make_scoring({"init": [2, -3, -60, -2, 0, 0, 0, 0, 0, 0]})

    def nw_checks(a, b):
        batch = W.from_pairs([(a, b)])
        (score, ra, rb), = ctx.nw_align_long(batch, nw)
        assert set(ctx.last_call()) <= {"long_forward", "long_block", "long_walk"}, ctx.last_call()
        assert ctx.last_call()["long_block"][0] >= 2, ctx.last_call()
        want = int(ctx.nw_score(batch, nw)[0])
        assert score == want, (score, want)
        assert rescore(ra, rb, 1, -2, -4, -1) == score
        assert ra.replace(b"-", b"") == a and rb.replace(b"-", b"") == b

    def sw_checks(a, b, oa, ob, n):
        batch = W.from_pairs([(a, b)])
        hits, = ctx.sw_align_long(batch, sw, 1)
        assert set(ctx.last_call()) <= {"long_forward", "long_block", "long_walk"}, ctx.last_call()
        s, ea, eb = ctx.sw_score(batch, sw)
        h, = hits
        assert (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) == (2 * n, oa, ob, n, n), h
        assert (int(s[0]), int(ea[0]), int(eb[0])) == (h["score"], h["pos_a"] + h["len_a"], h["pos_b"] + h["len_b"])
        assert h["a"] == h["b"] == a[oa:oa + n].decode()

    if which == "square":
        n = 60000
        a, b = related(rng, n, b"ACGT", 0.05)
        nw_checks(a, b)
        seg = np.frombuffer(b"ACGT", np.uint8)[rng.below(4, 3000).astype(np.int64)].tobytes()
        bg_a = np.frombuffer(b"AC", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
        bg_b = np.frombuffer(b"GT", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
        oa, ob = 21111, 38888
        sw_checks(bg_a[:oa] + seg + bg_a[oa + 3000:], bg_b[:ob] + seg + bg_b[ob + 3000:], oa, ob, 3000)
    else:
        n = 7200000
        a, b = related(rng, 300, b"ACGT", 0.1)
        bg = np.frombuffer(b"ACGT", np.uint8)[rng.below(4, n).astype(np.int64)].tobytes()
        nw_checks(a, bg[:3000000] + b + bg[3000000 + len(b):])
        seg = np.frombuffer(b"ACGT", np.uint8)[rng.below(4, 300).astype(np.int64)].tobytes()
        bg_b = np.frombuffer(b"GT", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
        ob = 5555555
        sw_checks(seg, bg_b[:ob] + seg + bg_b[ob + 300:], 0, ob, 300)
print("beyond-cap ok")
"""


def rescore(ra: bytes, rb: bytes, match: int, mismatch: int, gap_open: int, gap_extend: int) -> int:
    """Affine score of two gapped strings (plain scoring, no flags): a gap of length L costs gap_open + L * gap_extend."""
    x, y = np.frombuffer(ra, np.uint8), np.frombuffer(rb, np.uint8)
    ga, gb = x == ord("-"), y == ord("-")
    both = ~ga & ~gb
    s = int(np.where(x[both] == y[both], match, mismatch).sum())
    for g in (ga, gb):
        starts = int((g & ~np.concatenate(([False], g[:-1]))).sum())
        s += gap_open * starts + gap_extend * int(g.sum())
    return s


@pytest.mark.parametrize("which", ["square", "narrow"])
def test_beyond_the_cell_cap(which):
    """60 000 x 60 000 (3.6e9 cells) and 300 x 7 200 000 (just over 2^31): NW's score is nw_score's, a host rescoring of the
    strings gives it, the strings without gaps are the inputs; SW finds a planted segment exactly, with the score call's end.
    In a child process under a time limit."""
    out = subprocess.run([sys.executable, "-c", BEYOND_CAP, str(ROOT), which], capture_output=True, text=True, timeout=900,
                         cwd=str(ROOT / "tests"))
    assert out.returncode == 0 and "beyond-cap ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])


# ---------------------------------------------------------------- 5. errors, options, empty --
@pytest.mark.parametrize("is_sw", [0, 1])
def test_unknown_character_pair_is_named_as_the_score_calls_name_it(ctx, is_sw):
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    good = (b"ACGT" * 150, b"TTACGTACGTACGA" * 5)
    pairs = [good] * 12
    pairs[9] = (good[0], good[1][:20] + b"X" + good[1][21:])
    pairs[7] = (good[0][:7] + b"X" + good[0][8:], good[1])
    batch = W.from_pairs(pairs)
    score_call = ctx.sw_score if is_sw else ctx.nw_score
    with pytest.raises(S.SeqAlignError) as want:
        score_call(batch, hyb)
    for rows in (0, 16):
        with ctx.options(long_block_rows=rows), pytest.raises(S.SeqAlignError) as got:
            ctx.sw_align_long(batch, hyb, 1) if is_sw else ctx.nw_align_long(batch, hyb)
        assert got.value.code == want.value.code == S.E_UNKNOWN_PAIR
        assert "pair 7:" in str(got.value) and "pair 7:" in str(want.value), (str(got.value), str(want.value))


def test_domain_and_memory_errors(ctx):
    bad = S.make_scoring({"init": [1, -2, -4, -1, 0, 0, 1, 1, 0, 0]})   # both no_gaps: outside NW's parity domain
    batch = W.from_pairs([(b"ACGTACGT", b"ACGAACGT")])
    with pytest.raises(S.SeqAlignError) as want:
        ctx.nw_score(batch, bad)
    with pytest.raises(S.SeqAlignError) as got:
        ctx.nw_align_long(batch, bad)
    assert got.value.code == want.value.code == S.E_DOMAIN
    assert ctx.sw_align_long(batch, bad, 1) == ctx.sw_batch(batch, bad, 1, max_hits=1)   # SW: defined
    sc = S.make_scoring({"preset": "default"})
    big = W.from_pairs([(b"ACGT" * 600, b"ACGA" * 600)])
    with ctx.options(chunk_bytes=1 << 20):
        for call in (lambda: ctx.nw_align_long(big, sc), lambda: ctx.sw_align_long(big, sc, 1)):
            with pytest.raises(S.SeqAlignError) as e:
                call()
            assert e.value.code == S.E_NOMEM and "bytes" in str(e.value), str(e.value)
        small = W.from_pairs([(b"ACGT" * 40, b"ACGA" * 40)])
        check_nw(ctx, small, sc)                     # what fits still runs under the same budget


def test_sw_capacities(ctx):
    """hit_cap / str_cap too small: the hits that fit are delivered, then SEQALIGN_E_NOMEM -- as sw_batch."""
    import ctypes as C
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    batch = W.from_pairs([(b"ACGTACGTAA", b"ACGTACGTAA"), (b"GGGGCCCC", b"GGGGCCCC"), (b"TTTT", b"TTTT")])
    ms = np.ones(3, np.int32)
    for cap, scap in ((2, 1 << 10), (8, 15)):
        for fn in ("seqalign_sw_batch", "seqalign_sw_align_long"):
            hits, n_hits = (S.SwHit * 8)(), C.c_uint64(0)
            oa, ob = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
            d = S.batch_desc(batch)
            args = [ctx._h, C.byref(d), C.byref(sc), S._ptr(ms)] + ([C.c_uint32(1)] if fn == "seqalign_sw_batch" else []) + \
                   [hits, C.c_uint64(cap), C.byref(n_hits), S._ptr(oa), S._ptr(ob), C.c_uint64(scap)]
            rc = getattr(S.lib(), fn)(*args)
            listed = [(hits[k].pair, hits[k].score, hits[k].length, hits[k].str_off) for k in range(n_hits.value)]
            used = max([h[3] + h[2] + 1 for h in listed], default=0)
            got = (rc, n_hits.value, listed, oa[:used].tobytes(), ob[:used].tobytes())
            if fn == "seqalign_sw_batch":
                want = got
            else:
                assert got == want, (cap, scap, got, want)
        assert want[0] == S.E_NOMEM and want[1] == (2 if cap == 2 else 1)


def test_empty_sequences(ctx):
    sc = S.make_scoring({"preset": "default"})
    batch = W.from_pairs([(b"", b""), (b"ACGT", b""), (b"", b"ACGT"), (b"A", b"A"), (b"", b"")])
    for rows in (1, 0):
        with ctx.options(long_block_rows=rows):
            check_nw(ctx, batch, sc)
            check_sw(ctx, batch, sc, 1)
    assert ctx.nw_align_long(W.from_pairs([]), sc) == []


def test_long_block_rows_option(ctx):
    before = ctx.get_option("long_block_rows")
    for v in ("0", "5", "4294967295"):
        ctx.set_option("long_block_rows", v)
        assert ctx.get_option("long_block_rows") == v
    for v in ("abc", "-1", "1x", "", "4294967296", "2.5"):
        with pytest.raises(S.SeqAlignError):
            ctx.set_option("long_block_rows", v)
        assert ctx.get_option("long_block_rows") == "4294967295"
    ctx.set_option("long_block_rows", before)
