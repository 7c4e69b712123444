"""GPU tier: score only -- seqalign_nw_score_batch / seqalign_sw_score_batch (sa_score.hip, sa_batch_score.hip).

NW: the global score, max(match, gap_a, gap_b) of the last cell (needleman_wunsch.c:54-66).  SW: the best match_scores cell
in hit order -- score desc, column asc, row asc (smith_waterman.c:71-86) -- with its 1-based coordinates.
Checked against the oracle's matrices, the golden vectors, the existing calls, and beyond the 2^31-cell cap.
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


def want_from_matrices(M, A, B, la, lb, is_sw):
    """(score, end_a, end_b) the score-only call must return, from the three matrices of one pair."""
    if not is_sw:
        return int(max(M[-1], A[-1], B[-1])), 0, 0
    Mr = np.asarray(M, np.int64).reshape(lb + 1, la + 1)
    best = int(Mr.max())
    if best <= 0:
        return 0, 0, 0
    rows, cols = np.nonzero(Mr == best)
    k = np.lexsort((rows, cols))[0]          # column asc, then row asc
    return best, int(cols[k]), int(rows[k])


def oracle_want(osc, batch, is_sw):
    out = []
    for p in range(batch.n_pairs):
        a, b = batch.seq_a(p), batch.seq_b(p)
        rc, M, A, B = O.oracle_fill(osc, a, b, is_sw)
        assert rc == 0
        out.append(want_from_matrices(M, A, B, len(a), len(b), is_sw))
    return out


def got_of(ctx, batch, sc, is_sw):
    if is_sw:
        s, ea, eb = ctx.sw_score(batch, sc)
        return [(int(s[p]), int(ea[p]), int(eb[p])) for p in range(batch.n_pairs)]
    s = ctx.nw_score(batch, sc)
    return [(int(s[p]), 0, 0) for p in range(batch.n_pairs)]


def assert_vs_oracle(ctx, batch, sc, is_sw, tag=""):
    want = oracle_want(oracle_scoring_of(sc), batch, is_sw)
    got = got_of(ctx, batch, sc, is_sw)
    bad = [(p, got[p], want[p]) for p in range(batch.n_pairs) if got[p] != want[p]]
    assert not bad, (tag, bad[:5])


def rand_seq(rng, n, alpha):
    return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""


# ---------------------------------------------------------------- 1. golden + all flags --
@pytest.mark.parametrize("is_sw", [0, 1])
def test_golden_small_pairs(ctx, is_sw):
    """Every case of fill_small.json (the compiled reference's matrices, all flag combinations): the score (and the SW best
    cell) follows from the golden matrices; kat.json's NW pairs agree with the oracle and with their stated scores."""
    n = 0
    for case in load("fill_small.json")["cases"]:
        sc = S.make_scoring(case["scoring"])
        pairs = [(g["a"].encode(), g["b"].encode()) for g in case["pairs"]]
        batch = W.from_pairs(pairs)
        got = got_of(ctx, batch, sc, is_sw)
        for p, g in enumerate(case["pairs"]):
            m = g["sw" if is_sw else "nw"]
            want = want_from_matrices(m["M"], m["A"], m["B"], len(g["a"]), len(g["b"]), is_sw)
            assert got[p] == want, (case["scoring"], g["a"], g["b"], got[p], want)
            if not is_sw and "score" in m:
                assert got[p][0] == m["score"]
            n += 1
    assert n >= 100
    for v in load("kat.json")["sw" if is_sw else "nw"]:
        sc = S.make_scoring(v["scoring"])
        batch = W.from_pairs([(v["a"].encode(), v["b"].encode())])
        assert_vs_oracle(ctx, batch, sc, is_sw, v["src"])
        if not is_sw and "score" in v:
            assert int(ctx.nw_score(batch, sc)[0]) == v["score"]


@pytest.mark.parametrize("is_sw", [0, 1])
def test_all_flag_combinations_vs_oracle(ctx, is_sw):
    """The 32 combinations of the reference's five flags (the GENERAL row sweep), random ragged batches."""
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        sc = S.make_scoring(spec)
        batch = W.ragged(40, seed=700 + idx, max_len=140, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        assert_vs_oracle(ctx, batch, sc, is_sw, f"flags={flags}")


# ---------------------------------------------------------------- 2. every width --
SCORINGS = {
    "dna": ({"preset": "default"}, b"ACGT"),
    "dna_sw": ({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}, b"ACGT"),
    "blosum62": ({"preset": "BLOSUM62"}, b"ARNDCQEGHILKMFPSTWYV"),
    "ext_pos": ({"init": [2, -3, -2, 1, 0, 0, 0, 0, 0, 0]}, b"ACGT"),
}


@pytest.mark.parametrize("name", list(SCORINGS))
@pytest.mark.parametrize("is_sw", [0, 1])
def test_widths_across_cpl_and_strip_boundaries(ctx, name, is_sw):
    """len_a on both sides of every columns-per-lane step and of the one-wave / strips limit (1 024), ragged len_b; one batch
    per width and one batch that mixes them all (several launches in one call)."""
    spec, alpha = SCORINGS[name]
    sc = S.make_scoring(spec)
    rng = W.Rng(9000 + 31 * is_sw + len(name))
    mixed = []
    for la in (1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4097):
        lbs = [0, 1, 64, 65] + [int(x) for x in rng.below(260, 3)]
        pairs = [(rand_seq(rng, la, alpha), rand_seq(rng, lb, alpha)) for lb in lbs]
        if la > 3:   # a related pair: long runs of matches, a real optimum to find
            a = pairs[-1][0]
            pairs.append((a, a[la // 3: la // 3 + 200] + rand_seq(rng, 17, alpha)))
        mixed += pairs[2:5]
        assert_vs_oracle(ctx, W.from_pairs(pairs), sc, is_sw, f"{name} la={la}")
    assert_vs_oracle(ctx, W.from_pairs(mixed), sc, is_sw, f"{name} mixed")


# ---------------------------------------------------------------- 3. the existing calls --
@pytest.mark.parametrize("cfg,n", [("C2", 10000), ("C3", 2000), ("C4", 1000)])
def test_agrees_with_alignment_calls(ctx, cfg, n):
    """C2: nw_score == nw_batch's scores; C3 / C4: sw_score == the first hit of sw_batch(min_score = 1, max_hits = 1) --
    score, and end = pos + len."""
    c = load("configs.json")[cfg]
    sc = S.make_scoring(c["scoring"])
    batch = W.make(c["gen"], n, c["kwargs"])
    if not c["is_sw"]:
        _, _, _, _, out_score = ctx.nw_batch(batch, sc, raw=True)
        got = ctx.nw_score(batch, sc)
        assert np.array_equal(got, out_score)
        assert set(ctx.last_call()) == {"score_rows"}
        return
    hits = ctx.sw_batch(batch, sc, 1, max_hits=1)
    s, ea, eb = ctx.sw_score(batch, sc)
    assert set(ctx.last_call()) == {"score_rows"}
    for p in range(n):
        want = (0, 0, 0) if not hits[p] else (hits[p][0]["score"], hits[p][0]["pos_a"] + hits[p][0]["len_a"],
                                              hits[p][0]["pos_b"] + hits[p][0]["len_b"])
        assert (int(s[p]), int(ea[p]), int(eb[p])) == want, (cfg, p)


# ---------------------------------------------------------------- 4. unknown pair --
@pytest.mark.parametrize("is_sw", [0, 1])
def test_unknown_character_pair_names_the_lowest_pair(ctx, is_sw):
    """A character pair without a score (use_match_mismatch = 0: alignment_scoring.c:178-181) fails the call with
    SEQALIGN_E_UNKNOWN_PAIR and names the lowest failing pair -- the pair whose fill status is set, the call nw_batch fails
    on; narrow rows and strips alike."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    for width in (60, 1500):
        good = (b"ACGT" * (width // 4), b"TTACGTACGTACGA" * 5)
        pairs = [good] * 90
        bad_b = good[1][:20] + b"X" + good[1][21:]
        pairs[61] = (good[0], bad_b)
        pairs[40] = (good[0][:7] + b"X" + good[0][8:], good[1])
        batch = W.from_pairs(pairs)
        status = ctx.fill_batch(batch, hyb, is_sw, check=False)[-1]
        assert [p for p in range(len(pairs)) if status[p] != S.STATUS_OK] == [40, 61]
        with pytest.raises(S.SeqAlignError) as err:
            (ctx.sw_score if is_sw else ctx.nw_score)(batch, hyb)
        assert err.value.code == S.E_UNKNOWN_PAIR and "pair 40:" in str(err.value), str(err.value)
        if not is_sw:
            with pytest.raises(S.SeqAlignError) as err2:
                ctx.nw_batch(batch, hyb)
            assert err2.value.code == S.E_UNKNOWN_PAIR
        ok = W.from_pairs([good] * 5)   # the context still works
        got = ctx.sw_score(ok, hyb)[0] if is_sw else ctx.nw_score(ok, hyb)
        assert len(got) == 5 and len(set(got.tolist())) == 1


# ---------------------------------------------------------------- 4b. several chunks --
MIB = 1 << 20   # the smallest chunk_bytes the option accepts


def chunked_pairs(seed, strip_len_a, n=5000):
    """n pairs with both lengths drawn from 100 .. 300 (len_a + len_b + 64 bytes of a chunk each: three chunks of 1 MiB at
    least), and three pairs of the strips class (len_a from strip_len_a, len_b <= 200) first, in the middle and last, so that
    several chunks carry a strips launch."""
    rng = W.Rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seq = lambda k: letters[rng.below(4, k).astype(np.int64)].tobytes()
    lens = 100 + rng.below(201, 2 * n).astype(np.int64)
    pairs = [(seq(int(lens[2 * k])), seq(int(lens[2 * k + 1]))) for k in range(n)]
    strips = [(seq(la), seq(lb)) for la, lb in zip(strip_len_a, (200, 133, 57))]
    return [strips[0]] + pairs[:n // 2] + [strips[1]] + pairs[n // 2:] + [strips[2]]


@pytest.mark.parametrize("is_sw", [0, 1])
def test_several_chunks_equal_the_oracle(ctx, is_sw):
    """One batch of more than 2 MiB at chunk_bytes = 1 MiB: every pair equals the oracle, and the call launched more often
    than at the default budget (which is how the test knows the batch was cut)."""
    sc = S.make_scoring(SCORINGS["dna_sw" if is_sw else "dna"][0])
    batch = W.from_pairs(chunked_pairs(1717 + is_sw, (1025, 1600, 1301)))
    assert int(batch.len_a.sum()) + int(batch.len_b.sum()) + 64 * batch.n_pairs > 2 * MIB
    want = oracle_want(oracle_scoring_of(sc), batch, is_sw)
    whole = got_of(ctx, batch, sc, is_sw)
    at_default = ctx.last_call()
    with ctx.options(chunk_bytes=MIB):
        cut = got_of(ctx, batch, sc, is_sw)
        at_mib = ctx.last_call()
    print(f"score_rows / score_strips launches: default budget {at_default}, 1 MiB {at_mib}")
    for tag, got in (("default budget", whole), ("1 MiB", cut)):
        bad = [(p, got[p], want[p]) for p in range(batch.n_pairs) if got[p] != want[p]]
        assert not bad, (tag, len(bad), bad[:5])
    assert at_mib["score_rows"][0] > at_default["score_rows"][0], (at_mib, at_default)
    assert at_mib["score_strips"][0] > at_default["score_strips"][0] == 1, (at_mib, at_default)


@pytest.mark.parametrize("is_sw", [0, 1])
def test_unknown_character_pair_in_the_last_chunk(ctx, is_sw):
    """12 000 pairs of 194 bytes each are three chunks of 1 MiB (5 405 pairs fill one): an X in two pairs of the last chunk
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
                (ctx.sw_score if is_sw else ctx.nw_score)(batch, hyb)
            ran = ctx.last_call()
        assert err.value.code == S.E_UNKNOWN_PAIR and "pair 11000:" in str(err.value), str(err.value)
        assert ran["score_rows"][0] == 3 and ("score_strips" in ran) == bool(long_a), ran   # the failure came in the third chunk


def test_time_hook_refuses_a_batch_of_several_chunks(ctx):
    """seqalign_score_time_ms times the launches of ONE chunk: a batch of more than 1 MiB at chunk_bytes = 1 MiB is
    SEQALIGN_E_ARG with the hook's own message; at the default budget it returns `repeats` positive times."""
    sc = S.make_scoring({"preset": "default"})
    batch = W.from_pairs([(b"ACGT" * 50, b"TTACGTACGTACGA" * 10)] * 4000)   # 404 bytes per pair: 1.6 MB
    for is_sw in (0, 1):
        with ctx.options(chunk_bytes=MIB):
            with pytest.raises(S.SeqAlignError) as err:
                ctx.score_time_ms(batch, sc, is_sw, repeats=3)
        assert err.value.code == S.E_ARG and "seqalign_score_time_ms: the batch does not fit one chunk" in str(err.value), str(err.value)
        ms = ctx.score_time_ms(batch, sc, is_sw, repeats=3)
        assert len(ms) == 3 and all(float(t) > 0 for t in ms), ms


# ---------------------------------------------------------------- 5. beyond the cap --
BEYOND_CAP = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[1] + "/seq-align_amd/python", sys.argv[1] + "/tests"]
import seqalign_amd as S
from seqalign_amd import workloads as W
n = 60000
rng = W.Rng(60000)
a = np.frombuffer(b"ACGT", np.uint8)[rng.below(4, n).astype(np.int64)].tobytes()
with S.Context(0) as ctx:
    nw = S.make_scoring({"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]})
    big = W.from_pairs([(a, a)])
    try:
        ctx.nw_batch(big, nw)
        raise SystemExit("nw_batch accepted a pair of 3.6e9 cells")
    except S.SeqAlignError as e:
        assert e.code == S.E_TOO_LARGE, e
    s = ctx.nw_score(big, nw)
    assert int(s[0]) == n * 1, s
    assert set(ctx.last_call()) == {"score_strips"}, ctx.last_call()
    # SW: an identical segment of 3 000 planted in two backgrounds that share no letter (A/C against G/T): the best local
    # alignment is exactly the segment
    seg = np.frombuffer(b"ACGT", np.uint8)[rng.below(4, 3000).astype(np.int64)].tobytes()
    bg_a = np.frombuffer(b"AC", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
    bg_b = np.frombuffer(b"GT", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
    oa, ob = 21111, 38888
    sa = bg_a[:oa] + seg + bg_a[oa + 3000:]
    sb = bg_b[:ob] + seg + bg_b[ob + 3000:]
    sw = S.make_scoring({"init": [2, -3, -60, -2, 0, 0, 0, 0, 0, 0]})
    s, ea, eb = ctx.sw_score(W.from_pairs([(sa, sb)]), sw)
    assert (int(s[0]), int(ea[0]), int(eb[0])) == (3000 * 2, oa + 3000, ob + 3000), (s, ea, eb)
print("beyond-cap ok")
"""


def test_beyond_the_cell_cap():
    """One pair of 60 000 x 60 000 (3.6e9 cells): nw_batch refuses it (SEQALIGN_E_TOO_LARGE), score only does not -- NW of a = a
    is 60 000 x match; SW finds a planted 3 000-long identical segment and its end.  In a child process under a time limit."""
    out = subprocess.run([sys.executable, "-c", BEYOND_CAP, str(ROOT)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "beyond-cap ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])


# ---------------------------------------------------------------- 6. several contexts --
def test_multi_context_equals_single(ctx):
    """Two contexts of one device (the *_multi calls' ranges, sa_multi.hip): the results are the single-context call's."""
    batch = W.ragged(3000, seed=77, max_len=1400, lower_frac=0.1)
    sc_nw = S.make_scoring({"preset": "default"})
    sc_sw = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    with S.Context(0) as peer:
        assert np.array_equal(ctx.nw_score(batch, sc_nw, peers=[peer]), ctx.nw_score(batch, sc_nw))
        one = ctx.sw_score(batch, sc_sw)
        two = ctx.sw_score(batch, sc_sw, peers=[peer])
        assert all(np.array_equal(x, y) for x, y in zip(one, two))
    sample = W.from_pairs([(batch.seq_a(p), batch.seq_b(p)) for p in range(0, 3000, 150)])
    assert_vs_oracle(ctx, sample, sc_sw, 1, "multi sample")
