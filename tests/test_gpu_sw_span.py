"""GPU tier: SW hit spans -- seqalign_sw_span_batch (sa_span.hip, sa_batch_score.hip).

Per pair (score, pos_a, pos_b, len_a, len_b) of the first hit of sw_batch(min_score = 1, max_hits = 1): the hit the
reference's walk (tie order GAP_A, GAP_B, MATCH) finds from the best cell, carried forward beside the scores.  Every case is
checked against spanlib.want_spans (the oracle's first hit) on all five outputs.
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
import spanlib as SP
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"


def load(name):
    return json.loads((GOLD / name).read_text())


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


def oracle_scoring_of(sc):
    return O.Scoring.from_buffer_copy(bytes(sc))


def assert_vs_oracle(ctx, batch, sc, tag="", want=None):
    want = want if want is not None else SP.want_spans(oracle_scoring_of(sc), batch)
    got = SP.got_spans(ctx.sw_span(batch, sc))
    bad = [(p, got[p], want[p]) for p in range(batch.n_pairs) if got[p] != want[p]]
    assert not bad, (tag, len(bad), bad[:5])
    return want


def rand_seq(rng, n, alpha):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


# ---------------------------------------------------------------- 1. golden + known answers --
def test_golden_and_known_answer_pairs(ctx):
    """The SW pairs of fill_small.json (every flag combination the reference's matrices were recorded for) and kat.json's
    known answers, whose recorded first hit is checked too."""
    n = 0
    for case in load("fill_small.json")["cases"]:
        sc = S.make_scoring(case["scoring"])
        pairs = [(g["a"].encode(), g["b"].encode()) for g in case["pairs"] if "sw" in g]
        if pairs:
            assert_vs_oracle(ctx, W.from_pairs(pairs), sc, case["scoring"])
            n += len(pairs)
    assert n >= 100
    for v in load("kat.json")["sw"]:
        sc = S.make_scoring(v["scoring"])
        batch = W.from_pairs([(v["a"].encode(), v["b"].encode())])
        want = assert_vs_oracle(ctx, batch, sc, v["src"])
        ha, hb = v["hits"][0]                  # the recorded first hit's two strings: the span covers exactly their letters
        _, pos_a, pos_b, len_a, len_b = want[0]
        assert v["a"][pos_a:pos_a + len_a] == ha.replace("-", "") and v["b"][pos_b:pos_b + len_b] == hb.replace("-", "")


# ---------------------------------------------------------------- 2. all flags --
def test_all_flag_combinations_vs_oracle(ctx):
    """The 32 combinations of the reference's five flags (the GENERAL sweep), test_gpu_score.py's specs and batches."""
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        sc = S.make_scoring(spec)
        batch = W.ragged(40, seed=700 + idx, max_len=140, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        assert_vs_oracle(ctx, batch, sc, f"flags={flags}")


# ---------------------------------------------------------------- 3. every width --
SCORINGS = {
    "dna_sw": ({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}, b"ACGT"),
    "blosum62": ({"preset": "BLOSUM62"}, b"ARNDCQEGHILKMFPSTWYV"),
    "ext_pos": ({"init": [2, -3, -2, 1, 0, 0, 0, 0, 0, 0]}, b"ACGT"),
}
# the issue's widths, and both sides of every class boundary of the span launcher: columns per lane 1, 2, 3, 4, 5, 6, 8 (64,
# 128, 192, 256, 320, 384 columns), one wave up to 512 columns, strips of 512 beyond
WIDTHS = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 511, 512, 513, 1023, 1024, 1025, 4097)


@pytest.mark.parametrize("name", list(SCORINGS))
def test_widths_across_cpl_and_strip_boundaries(ctx, name):
    spec, alpha = SCORINGS[name]
    sc = S.make_scoring(spec)
    rng = W.Rng(9100 + len(name))
    mixed = []
    for la in WIDTHS:
        lbs = [0, 1, 64, 65] + [int(x) for x in rng.below(260, 3)]
        pairs = [(rand_seq(rng, la, alpha), rand_seq(rng, lb, alpha)) for lb in lbs]
        if la > 3:   # a related pair: long runs of matches, a real hit to follow
            a = pairs[-1][0]
            pairs.append((a, a[la // 3: la // 3 + 200] + rand_seq(rng, 17, alpha)))
        mixed += pairs[2:5] + pairs[-1:]
        assert_vs_oracle(ctx, W.from_pairs(pairs), sc, f"{name} la={la}")
    assert_vs_oracle(ctx, W.from_pairs(mixed), sc, f"{name} mixed")   # every class in one call: several launches
    assert set(ctx.last_call()) == {"score_rows", "score_strips"}


# ---------------------------------------------------------------- 4. ties --
def indel_relative(rng, s, alpha):
    out = bytearray()
    for ch in s:
        r = int(rng.below(12, 1)[0])
        if r == 0:
            continue                                     # deletion
        if r == 1:
            out += rand_seq(rng, 1 + int(rng.below(3, 1)[0]), alpha)   # insertion
        out.append(ch)
    return bytes(out)


@pytest.mark.parametrize("init", [[2, -1, 0, -1], [3, -1, -1, 0]], ids=["open0", "ext0"])
def test_ties_follow_the_walkers_order(ctx, init):
    """200 pairs over a binary alphabet, half of them related by indels, scorings dense in ties.  First, on the CPU: at
    least 5 % of the pairs give another span when the predecessor priority is reversed (M > B > A), so a kernel with the
    wrong tie order cannot pass."""
    rng = W.Rng(4242 + init[0])
    pairs = []
    for k in range(200):
        la, lb = (1 + int(x) for x in rng.below(140, 2))
        a = rand_seq(rng, la, b"AC")
        pairs.append((a, indel_relative(rng, a, b"AC")[:140] if k % 2 else rand_seq(rng, lb, b"AC")))
    batch = W.from_pairs(pairs)
    sc = S.make_scoring({"init": init + [0] * 6})
    osc = oracle_scoring_of(sc)
    sensitive = SP.tie_sensitive(osc, batch)
    print(f"tie_sensitive {sensitive} of {batch.n_pairs}")
    assert sensitive >= batch.n_pairs // 20, sensitive
    assert_vs_oracle(ctx, batch, sc, f"ties {init}")


# ---------------------------------------------------------------- 5. seams --
SEAM_SC = {"init": [2, -3, -2, -1, 0, 0, 0, 0, 0, 0]}


def planted(rng, la, lb, pieces_a, pieces_b):
    """seq_a over A/C, seq_b over G/T (no letter in common), with pieces written in at the given offsets."""
    a, b = bytearray(rand_seq(rng, la, b"AC")), bytearray(rand_seq(rng, lb, b"GT"))
    for off, s in pieces_a:
        a[off:off + len(s)] = s
    for off, s in pieces_b:
        b[off:off + len(s)] = s
    assert len(a) == la and len(b) == lb
    return bytes(a), bytes(b)


def test_spans_across_strips_and_handoff_blocks(ctx):
    """Planted hits in the strips class (rows over 512 columns): known by construction, confirmed by the oracle."""
    rng = W.Rng(5150)
    seg = lambda n: rand_seq(rng, n, b"ACGT")
    sc = S.make_scoring(SEAM_SC)
    pairs, known = [], {}
    # (a) a hit that starts three strips left of where it ends: columns 301 .. 1 600
    s = seg(1300)
    pairs.append(planted(rng, 2000, 1400, [(300, s)], [(50, s)]))
    known[0] = (2600, 300, 50, 1300, 1300)
    # (b) a horizontal gap run of 40 columns over the strip boundary at 512: seq_a carries 40 letters seq_b lacks
    s1, s2, ins = seg(200), seg(200), rand_seq(rng, 40, b"AC")
    pairs.append(planted(rng, 1100, 700, [(292, s1 + ins + s2)], [(120, s1 + s2)]))
    known[1] = (800 - 2 - 40, 292, 120, 440, 400)
    # (c) a vertical gap run of 30 rows over the hand-off block boundary at row 128, in the second strip
    s1, s2, ins = seg(60), seg(200), rand_seq(rng, 30, b"GT")
    pairs.append(planted(rng, 1100, 500, [(600, s1 + s2)], [(53, s1 + ins + s2)]))
    known[2] = (520 - 2 - 30, 600, 53, 260, 290)
    # (d) a hit longer than 64 rows inside one strip
    s = seg(300)
    pairs.append(planted(rng, 1100, 600, [(560, s)], [(200, s)]))
    known[3] = (600, 560, 200, 300, 300)
    # (e) two hits of equal score, in two strips and on the same rows: the one in the lower column is the first hit
    s = seg(150)
    pairs.append(planted(rng, 1600, 400, [(1300, s), (100, s)], [(77, s)]))
    known[4] = (300, 100, 77, 150, 150)
    assert all(max(len(a), len(b)) <= 3000 and len(b) <= 1500 for a, b in pairs)
    batch = W.from_pairs(pairs)
    want = SP.want_spans(oracle_scoring_of(sc), batch)
    assert all(want[p] == known[p] for p in known), [(want[p], known[p]) for p in known]
    assert_vs_oracle(ctx, batch, sc, "seams", want)
    assert set(ctx.last_call()) == {"score_strips"}


# ---------------------------------------------------------------- 6. the alignment call --
@pytest.mark.parametrize("cfg,n", [("C3", 2000), ("C4", 1000)])
def test_agrees_with_the_alignment_call(ctx, cfg, n):
    """sw_span == the first hit of sw_batch(min_score = 1, max_hits = 1), field for field."""
    c = load("configs.json")[cfg]
    sc = S.make_scoring(c["scoring"])
    batch = W.make(c["gen"], n, c["kwargs"])
    hits = ctx.sw_batch(batch, sc, 1, max_hits=1)
    got = SP.got_spans(ctx.sw_span(batch, sc))
    assert set(ctx.last_call()) == {"score_rows"}
    for p in range(n):
        h = hits[p][0] if hits[p] else None
        want = (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) if h else (0, 0, 0, 0, 0)
        assert got[p] == want, (cfg, p, got[p], want)


# ---------------------------------------------------------------- 7. unknown pair --
def test_unknown_character_pair_names_the_lowest_pair(ctx):
    """test_gpu_score.py's scoring and batch: the same code and the same pair named as the score call; narrow rows and
    strips alike."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    for width in (60, 1500):
        good = (b"ACGT" * (width // 4), b"TTACGTACGTACGA" * 5)
        pairs = [good] * 90
        bad_b = good[1][:20] + b"X" + good[1][21:]
        pairs[61] = (good[0], bad_b)
        pairs[40] = (good[0][:7] + b"X" + good[0][8:], good[1])
        batch = W.from_pairs(pairs)
        with pytest.raises(S.SeqAlignError) as ref:
            ctx.sw_score(batch, hyb)
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_span(batch, hyb)
        assert err.value.code == ref.value.code == S.E_UNKNOWN_PAIR
        assert "pair 40:" in str(err.value) and "pair 40:" in str(ref.value), (str(err.value), str(ref.value))
        ok = W.from_pairs([good] * 5)   # the context still works
        assert_vs_oracle(ctx, ok, hyb, f"after the failure, width {width}")


# ---------------------------------------------------------------- 7b. several chunks --
MIB = 1 << 20   # the smallest chunk_bytes the option accepts


def chunked_pairs(seed, strip_len_a, n=5000):
    """test_gpu_score.py's batch: n pairs with both lengths drawn from 100 .. 300 (len_a + len_b + 72 bytes of a chunk each:
    three chunks of 1 MiB at least), and three pairs of the strips class (len_a from strip_len_a, len_b <= 200; about 20 KB
    each) first, in the middle and last, so that several chunks carry a strips launch."""
    rng = W.Rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seq = lambda k: letters[rng.below(4, k).astype(np.int64)].tobytes()
    lens = 100 + rng.below(201, 2 * n).astype(np.int64)
    pairs = [(seq(int(lens[2 * k])), seq(int(lens[2 * k + 1]))) for k in range(n)]
    strips = [(seq(la), seq(lb)) for la, lb in zip(strip_len_a, (200, 133, 57))]
    return [strips[0]] + pairs[:n // 2] + [strips[1]] + pairs[n // 2:] + [strips[2]]


def test_several_chunks_equal_the_oracle(ctx):
    """One batch of more than 2 MiB at chunk_bytes = 1 MiB: every pair equals the reference's first hit, and the call launched
    more often than at the default budget (which is how the test knows the batch was cut)."""
    sc = S.make_scoring(SCORINGS["dna_sw"][0])
    batch = W.from_pairs(chunked_pairs(2727, (600, 1600, 1111)))
    assert int(batch.len_a.sum()) + int(batch.len_b.sum()) + 72 * batch.n_pairs > 2 * MIB
    want = assert_vs_oracle(ctx, batch, sc, "default budget")
    at_default = ctx.last_call()
    with ctx.options(chunk_bytes=MIB):
        assert_vs_oracle(ctx, batch, sc, "1 MiB", want)
        at_mib = ctx.last_call()
    print(f"score_rows / score_strips launches: default budget {at_default}, 1 MiB {at_mib}")
    assert at_mib["score_rows"][0] > at_default["score_rows"][0], (at_mib, at_default)
    assert at_mib["score_strips"][0] > at_default["score_strips"][0] == 1, (at_mib, at_default)


def test_unknown_character_pair_in_the_last_chunk(ctx):
    """12 000 pairs of 202 bytes each are three chunks of 1 MiB (5 190 pairs fill one): an X in two pairs of the last chunk
    names the lower one by its number in the whole batch -- first in a narrow pair, then in a pair of the strips class."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    good = (b"ACGT" * 15, b"TTACGTACGTACGA" * 5)
    for long_a in (0, 1500):
        pairs = [good] * 12000
        bad_a = b"ACGT" * (long_a // 4) if long_a else good[0]
        pairs[11000] = (bad_a[:7] + b"X" + bad_a[8:], good[1])
        pairs[11500] = (good[0], good[1][:20] + b"X" + good[1][21:])
        batch = W.from_pairs(pairs)
        with ctx.options(chunk_bytes=MIB):
            with pytest.raises(S.SeqAlignError) as err:
                ctx.sw_span(batch, hyb)
            ran = ctx.last_call()
        assert err.value.code == S.E_UNKNOWN_PAIR and "pair 11000:" in str(err.value), str(err.value)
        assert ran["score_rows"][0] == 3 and ("score_strips" in ran) == bool(long_a), ran   # the failure came in the third chunk


def test_time_hook_refuses_a_batch_of_several_chunks(ctx):
    """seqalign_sw_span_time_ms times the launches of ONE chunk: a batch of more than 1 MiB at chunk_bytes = 1 MiB is
    SEQALIGN_E_ARG with the hook's own message; at the default budget it returns `repeats` positive times."""
    sc = S.make_scoring(SCORINGS["dna_sw"][0])
    batch = W.from_pairs([(b"ACGT" * 50, b"TTACGTACGTACGA" * 10)] * 4000)   # 412 bytes per pair: 1.6 MB
    with ctx.options(chunk_bytes=MIB):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_span_time_ms(batch, sc, repeats=3)
    assert err.value.code == S.E_ARG and "seqalign_sw_span_time_ms: the batch does not fit one chunk" in str(err.value), str(err.value)
    ms = ctx.sw_span_time_ms(batch, sc, repeats=3)
    assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms


# ---------------------------------------------------------------- 8. beyond the cap --
BEYOND_CAP = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[1] + "/seq-align_amd/python", sys.argv[1] + "/tests"]
import seqalign_amd as S
from seqalign_amd import workloads as W
n = 60000
rng = W.Rng(60000)
with S.Context(0) as ctx:
    # an identical segment of 3 000 planted in two backgrounds that share no letter (A/C against G/T): the best local
    # alignment is exactly the segment
    seg = np.frombuffer(b"ACGT", np.uint8)[rng.below(4, 3000).astype(np.int64)].tobytes()
    bg_a = np.frombuffer(b"AC", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
    bg_b = np.frombuffer(b"GT", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
    oa, ob = 21111, 38888
    sa = bg_a[:oa] + seg + bg_a[oa + 3000:]
    sb = bg_b[:ob] + seg + bg_b[ob + 3000:]
    sw = S.make_scoring({"init": [2, -3, -60, -2, 0, 0, 0, 0, 0, 0]})
    got = tuple(int(x[0]) for x in ctx.sw_span(W.from_pairs([(sa, sb)]), sw))
    assert got == (6000, 21111, 38888, 3000, 3000), got
    assert set(ctx.last_call()) == {"score_strips"}, ctx.last_call()
print("beyond-cap ok")
"""


def test_beyond_the_cell_cap():
    """One pair of 60 000 x 60 000 (3.6e9 cells, past the alignment calls' cap): the planted 3 000-long segment's score,
    start and lengths.  In a child process under a time limit."""
    out = subprocess.run([sys.executable, "-c", BEYOND_CAP, str(ROOT)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "beyond-cap ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])


# ---------------------------------------------------------------- 9. several contexts --
def test_multi_context_equals_single(ctx):
    """Two contexts of one device (sa_multi.hip's cell-balanced ranges): the results are the single-context call's."""
    batch = W.ragged(3000, seed=77, max_len=1400, lower_frac=0.1)
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    with S.Context(0) as peer:
        one = ctx.sw_span(batch, sc)
        two = ctx.sw_span(batch, sc, peers=[peer])
        assert all(np.array_equal(x, y) for x, y in zip(one, two))
    sample = W.from_pairs([(batch.seq_a(p), batch.seq_b(p)) for p in range(0, 3000, 150)])
    assert_vs_oracle(ctx, sample, sc, "multi sample")
