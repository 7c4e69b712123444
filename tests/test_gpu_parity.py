"""GPU parity tests: the HIP path, called through the C-ABI, against the oracle
and the committed golden vectors.  Bit-exact int32 everywhere (integer work).

Run on an MI355X:  python -m pytest tests -m gpu -x -q
"""
import ctypes as C
import itertools
import json
import os
import time
from pathlib import Path

import numpy as np
import pytest

import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
KERNELS = [S.KERNEL_WAVEFRONT, S.KERNEL_ROWSCAN, S.KERNEL_STREAM, S.KERNEL_STRIPS, S.KERNEL_WGSTREAM]
KID = lambda k: S.KERNEL_NAMES[k]


def load(name):
    return json.loads((GOLD / name).read_text())


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


@pytest.fixture
def opts(ctx):
    """Set options on the module's context for ONE test (seqalign_ctx_set_option: a context's choices are its
    own options, not process environment); the defaults come back afterwards."""
    changed = []

    def set_(**kv):
        for k, v in kv.items():
            ctx.set_option(k, v)
            changed.append(k)
    yield set_
    for k in changed:
        ctx.set_option(k, S.OPTION_DEFAULTS[k])


def oracle_scoring_of(sc: S.Scoring) -> O.Scoring:
    return O.Scoring.from_buffer_copy(bytes(sc))


def device_fill(ctx, batch, sc, is_sw, kernel, poison=True):
    import torch
    h = ctx.upload_scoring(sc, is_sw)
    db = S.DeviceBatch(batch, 0)
    if poison:
        for t in (db.M, db.A, db.B):
            t.fill_(0x5A5A5A5A)
    db.fill(ctx, h, kernel)
    torch.cuda.synchronize()
    ctx.release_scoring(h)
    return db


def assert_pairs_match_oracle(db, batch, osc, is_sw, pairs, tag=""):
    for p in pairs:
        rc, M, A, B = O.oracle_fill(osc, batch.seq_a(p), batch.seq_b(p), is_sw)
        assert rc == 0
        gM, gA, gB = db.pair_matrices(p)
        for name, g, w in (("M", gM, M), ("A", gA, A), ("B", gB, B)):
            if not np.array_equal(g, w):
                bad = int(np.nonzero(g != w)[0][0])
                Wd = len(batch.seq_a(p)) + 1
                raise AssertionError(f"{tag} pair {p} matrix {name} first diff at cell {bad} "
                                     f"(i={bad % Wd}, j={bad // Wd}): gpu {g[bad]} oracle {w[bad]}; "
                                     f"a={batch.seq_a(p)!r} b={batch.seq_b(p)!r}")


# ------------------------------------------------------------------ hardware --
def test_dpp_wave_shr1_is_a_full_wave_shift(ctx):
    """The kernels rely on v_mov_b32_dpp wave_shr:1 shifting across all 64 lanes."""
    out = ctx.dpp_probe(fill=-7)
    want = np.concatenate([[-7], np.arange(63) * 3 + 1]).astype(np.int32)
    assert np.array_equal(out, want), out


# -------------------------------------------------------------- golden vectors --
@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_reference_known_answer_matrices(ctx, kernel):
    """README.md:118-145: every cell of the three matrices, incl. the NW floor."""
    v = [x for x in load("kat.json")["nw"] if "match_scores" in x][0]
    sc = S.make_scoring(v["scoring"])
    batch = W.from_pairs([(v["a"].encode(), v["b"].encode())])
    db = device_fill(ctx, batch, sc, 0, kernel)
    M, A, B = db.pair_matrices(0)
    assert M.tolist() == sum(v["match_scores"], [])
    assert A.tolist() == sum(v["gap_a_scores"], [])
    assert B.tolist() == sum(v["gap_b_scores"], [])


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_fill_small_golden_all_flag_combinations(ctx, kernel):
    """Matrices produced by the compiled reference for all 32 flag combinations."""
    n = 0
    for case in load("fill_small.json")["cases"]:
        sc = S.make_scoring(case["scoring"])
        for key, is_sw in (("nw", 0), ("sw", 1)):
            pairs = [p for p in case["pairs"] if key in p]
            if not pairs:
                continue
            batch = W.from_pairs([(p["a"].encode(), p["b"].encode()) for p in pairs])
            db = device_fill(ctx, batch, sc, is_sw, kernel)
            for k, p in enumerate(pairs):
                M, A, B = db.pair_matrices(k)
                assert (M.tolist(), A.tolist(), B.tolist()) == (p[key]["M"], p[key]["A"], p[key]["B"]), \
                    (case["scoring"], p["a"], p["b"], key)
                n += 1
            assert (db.status.cpu().numpy() == -1).all()
    assert n > 250


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
@pytest.mark.parametrize("name", ["C2", "C2_related", "C3", "C4", "C5", "C5_rank7"])
def test_config_golden_digests(ctx, kernel, name):
    """64 seeded pairs per BASELINE config: FNV digests from the compiled reference."""
    cfg = load("configs.json")[name]
    sc = S.make_scoring(cfg["scoring"])
    batch = W.make(cfg["gen"], cfg["n"], cfg["kwargs"])
    db = device_fill(ctx, batch, sc, cfg["is_sw"], kernel)
    for p, g in enumerate(cfg["pairs"]):
        M, A, B = db.pair_matrices(p)
        assert (f"{O.fnv(M):016x}", f"{O.fnv(A):016x}", f"{O.fnv(B):016x}") == (g["M"], g["A"], g["B"]), (name, p)


# ------------------------------------------------------- differential vs oracle --
@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
@pytest.mark.parametrize("is_sw", [0, 1])
def test_all_flag_combinations_vs_oracle(ctx, kernel, is_sw):
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        mismatch = -6 if (flags[2] and flags[3]) else -2
        spec = {"init": [1, mismatch, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else [],
                "mutations": [["a", "c", -3], ["c", "a", 2]] if idx % 4 == 1 else []}
        sc = S.make_scoring(spec)
        batch = W.ragged(24, seed=300 + idx, max_len=90, lower_frac=0.2,
                         extra=b"N" if spec["wildcards"] else b"")
        db = device_fill(ctx, batch, sc, is_sw, kernel)
        assert_pairs_match_oracle(db, batch, oracle_scoring_of(sc), is_sw, range(batch.n_pairs),
                                  tag=f"{KID(kernel)} flags={flags}")


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
@pytest.mark.parametrize("max_len,n", [(1, 16), (64, 32), (65, 32), (200, 24), (330, 12), (700, 8), (1300, 4)])
def test_ragged_lengths_and_column_strips(ctx, kernel, max_len, n):
    """Empty sequences, every columns-per-lane instantiation, and (len_a > 512)
    the multi-strip path whose left boundary is read back from the matrices."""
    for is_sw, spec in ((0, {"preset": "default"}), (1, {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}),
                        (0, {"init": [1, -2, -4, -1, 1, 1, 0, 0, 0, 0]})):
        sc = S.make_scoring(spec)
        batch = W.ragged(n, seed=max_len * 7 + is_sw, max_len=max_len, lower_frac=0.1)
        # force the extremes into the batch
        fixed = [(b"", b""), (b"A", b""), (b"", b"ACGT"), (b"ACGT" * (max_len // 4), b"ACGT" * (max_len // 4))]
        pairs = [(batch.seq_a(p), batch.seq_b(p)) for p in range(batch.n_pairs)] + fixed
        batch = W.from_pairs(pairs)
        db = device_fill(ctx, batch, sc, is_sw, kernel)
        assert_pairs_match_oracle(db, batch, oracle_scoring_of(sc), is_sw, range(batch.n_pairs),
                                  tag=f"{KID(kernel)} max_len={max_len} sw={is_sw}")


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_protein_presets_vs_oracle(ctx, kernel):
    for preset, is_sw in (("BLOSUM62", 1), ("BLOSUM62", 0), ("PAM30", 1), ("BLOSUM80", 0), ("PAM70", 1)):
        sc = S.make_scoring({"preset": preset})
        batch = W.ragged(12, seed=len(preset) + is_sw, max_len=320, alphabet=b"ARNDCQEGHILKMFPSTWYVBZX",
                         lower_frac=0.2, extra=b"J*")
        db = device_fill(ctx, batch, sc, is_sw, kernel)
        assert_pairs_match_oracle(db, batch, oracle_scoring_of(sc), is_sw, range(batch.n_pairs),
                                  tag=f"{KID(kernel)} {preset}")


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_unknown_pair_is_reported_per_pair(ctx, kernel):
    """use_match_mismatch off + a pair missing from the table: the reference exit()s
    at the first such cell in row-major order; we report that cell index."""
    sc = S.make_scoring({"preset": "DNA_hybridization"})
    pairs = [(b"ACGT", b"ACGT"), (b"ACGTN", b"ACGT"), (b"ACGT", b"AXGT"), (b"AC", b"GT")]
    batch = W.from_pairs(pairs)
    db = device_fill(ctx, batch, sc, 0, kernel)
    st = db.status.cpu().numpy().view(np.uint64)
    assert st[0] == S.STATUS_OK and st[3] == S.STATUS_OK
    assert st[1] == 1 * 6 + 5          # row 1, column 5 ('N' is a[4])
    assert st[2] == 2 * 5 + 1          # row 2 ('X' is b[1]), column 1
    osc = oracle_scoring_of(sc)
    assert_pairs_match_oracle(db, batch, osc, 0, [0, 3])


def test_wide_alphabet_uses_the_global_table(ctx):
    """> 64 classes: substitution table stays in global memory (SA_SUBST_GLOBAL)."""
    letters = [chr(c) for c in range(33, 33 + 70)]
    muts = [[x, y, ((ord(x) * 7 + ord(y) * 3) % 11) - 5] for x in letters for y in letters]
    spec = {"init": [1, -6, -4, -1, 0, 0, 0, 0, 0, 1], "mutations": muts}
    sc = S.make_scoring(spec)
    batch = W.ragged(10, seed=5, max_len=100, alphabet="".join(letters).encode() + b"~")
    for kernel in KERNELS:
        for is_sw in (0, 1):
            db = device_fill(ctx, batch, sc, is_sw, kernel)
            assert_pairs_match_oracle(db, batch, oracle_scoring_of(sc), is_sw, range(batch.n_pairs))


# ------------------------------------------------------------ full-size configs --
FULL = {
    "C2": dict(gen=W.dna_nw_150, n=10000, kwargs=dict(seed=1), is_sw=0, scoring={"preset": "default"}),
    "C3": dict(gen=W.dna_sw_read_vs_ref, n=10000, kwargs=dict(seed=2), is_sw=1,
               scoring={"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}),
    "C4": dict(gen=W.protein_sw_300, n=4000, kwargs=dict(seed=3), is_sw=1, scoring={"preset": "BLOSUM62"}),
    # BASELINE configs[4]: 1 M pairs over 8 GPUs = 125 000 pairs (34 GB of matrices) per GPU; rank 7's share
    "C5": dict(gen=lambda n, **kw: W.dna_nw_indexed(875000, n, **kw), n=125000, kwargs=dict(seed=5), is_sw=0,
               scoring={"preset": "default"}),
}


@pytest.mark.parametrize("name", list(FULL))
def test_full_size_config_properties(ctx, name):
    """BASELINE sizes: (1) the three independently scheduled kernels agree on every
    byte (incl. the untouched padding between pairs), (2) a strided sample equals the oracle, (3) SW: the reduction kernel's
    best cell equals max(M) in reference hit order, (4) NW: last-cell scores equal
    the host traceback's, (5) duplicated pairs give identical matrices."""
    import torch
    cfg = FULL[name]
    sc = S.make_scoring(cfg["scoring"])
    osc = oracle_scoring_of(sc)
    batch = cfg["gen"](cfg["n"], **cfg["kwargs"])
    # property 5: make the last 8 pairs copies of the first 8
    for k in range(8):
        batch.off_a[-1 - k], batch.off_b[-1 - k] = batch.off_a[k], batch.off_b[k]
    db1 = device_fill(ctx, batch, sc, cfg["is_sw"], S.KERNEL_WAVEFRONT)
    sums1 = [int(t.to(torch.int64).sum().item()) for t in (db1.M, db1.A, db1.B)]
    M1 = db1.M.clone(); A1 = db1.A.clone(); B1 = db1.B.clone()   # (C5: 3 x 11.4 GB, twice -- 288 GB of HBM)
    del db1
    for other in (S.KERNEL_ROWSCAN, S.KERNEL_STREAM):
        db2 = device_fill(ctx, batch, sc, cfg["is_sw"], other)
        # padding cells between pairs keep the poison in every run, so whole arenas compare
        assert torch.equal(M1, db2.M) and torch.equal(A1, db2.A) and torch.equal(B1, db2.B), KID(other)
        assert sums1 == [int(t.to(torch.int64).sum().item()) for t in (db2.M, db2.A, db2.B)]
        if other != S.KERNEL_STREAM:
            del db2
    del M1, A1, B1
    sample = list(range(0, batch.n_pairs, max(1, batch.n_pairs // 48)))
    assert_pairs_match_oracle(db2, batch, osc, cfg["is_sw"], sample, tag=name)
    for k in range(8):
        for x, y in zip(db2.pair_matrices(k), db2.pair_matrices(batch.n_pairs - 1 - k)):
            assert np.array_equal(x, y)
    assert (db2.status.cpu().numpy() == -1).all()
    if cfg["is_sw"]:
        best_s, best_i, count, _ = db2.sw_reduce(ctx, min_score=60, with_candidates=False)
        for p in sample:
            M, _, _ = db2.pair_matrices(p)
            Wd = int(batch.len_a[p]) + 1
            assert best_s[p] == M.max()
            idx = np.nonzero(M == M.max())[0]
            cols = idx % Wd
            want = idx[np.lexsort((idx, cols))][0] if M.max() > 0 else 0
            assert best_i[p] == want
            assert count[p] == int((M >= 60).sum())
    else:
        last = torch.from_numpy((db2.mat_off_host + db2.cells_host.astype(np.uint64) - 1).astype(np.int64)).cuda()
        end = torch.maximum(torch.maximum(db2.M[last], db2.A[last]), db2.B[last]).cpu().numpy()
        for p in sample:
            rc, s, _, _ = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and s == end[p]
        if name == "C5":
            # the share through the host-level call (H2D -> fill -> device traceback -> strings): the head of
            # the share equals the compiled reference's strings (golden), a strided sample equals the oracle's
            del db2
            gold = load("configs.json")["C5_rank7"]["pairs"]
            str_off, out_a, out_b, out_len, out_score = ctx.nw_batch(batch, sc, raw=True)

            def got(p):
                o, ln = int(str_off[p]), int(out_len[p])
                return int(out_score[p]), out_a[o:o + ln].tobytes(), out_b[o:o + ln].tobytes()
            for p, g in enumerate(gold):
                assert got(p) == (g["score"], g["result_a"].encode(), g["result_b"].encode()), p
            for p in list(range(8, batch.n_pairs, batch.n_pairs // 200)) + [batch.n_pairs - 9]:
                rc, s, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
                assert rc == 0 and got(p) == (s, ra, rb), p
            for k in range(8):   # the duplicated pairs
                assert got(k) == got(batch.n_pairs - 1 - k)


@pytest.mark.parametrize("kernel", [S.KERNEL_AUTO] + KERNELS, ids=KID)
def test_positive_gap_extend(ctx, kernel):
    """gap_extend > 0 (legal upstream: scoring_init takes any int, alignment_scoring.c:21-55).  The row sweeps'
    gap_b scan takes its trend from the right end for a positive extension (sa_rowsweep.hpp: t(g) = (G - g) ext),
    so every kernel serves the request itself (until round 3 all of them were routed to the anti-diagonal kernel);
    the matrices must be the reference recurrence's, and so must the alignments built from them."""
    for spec in ({"init": [1, -2, -4, 1, 0, 0, 0, 0, 0, 0]}, {"init": [2, -3, -6, 2, 0, 1, 0, 0, 0, 0]},
                 {"init": [1, -1, 0, 3, 1, 0, 0, 0, 0, 1]}):
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        batch = W.ragged(20, seed=spec["init"][3] * 11 + 1, max_len=130, lower_frac=0.2)
        for is_sw in (0, 1):
            db = device_fill(ctx, batch, sc, is_sw, kernel)
            assert_pairs_match_oracle(db, batch, osc, is_sw, range(batch.n_pairs), tag=f"ext>0 {KID(kernel)} {spec}")
    if kernel == S.KERNEL_AUTO:   # end to end: both device walkers' decision order with a positive extension
        sc = S.make_scoring({"init": [1, -2, -4, 1, 0, 0, 0, 0, 0, 0]})
        osc = oracle_scoring_of(sc)
        batch = W.ragged(30, seed=8, max_len=90)
        res = ctx.nw_batch(batch, sc)
        got1, got5 = ctx.sw_batch(batch, sc, 5, max_hits=1), ctx.sw_batch(batch, sc, 5, max_hits=5)
        for p in range(batch.n_pairs):
            rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and res[p] == (s_, ra, rb), p
            for got, mh in ((got1, 1), (got5, 5)):
                rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), 5, mh)
                assert rc == 0 and got[p] == want, (p, mh)


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_transpose_symmetry(ctx, kernel):
    """Symmetric scoring: swapping a and b transposes the matrices and swaps
    gap_a <-> gap_b (a size-independent property of the recurrence)."""
    sc = S.make_scoring({"preset": "default"})
    batch = W.ragged(16, seed=99, max_len=180)
    swapped = W.Batch(batch.arena, batch.off_b, batch.len_b, batch.off_a, batch.len_a)
    for is_sw in (0, 1):
        d1, d2 = device_fill(ctx, batch, sc, is_sw, kernel), device_fill(ctx, swapped, sc, is_sw, kernel)
        for p in range(batch.n_pairs):
            la, lb = int(batch.len_a[p]), int(batch.len_b[p])
            M1, A1, B1 = (x.reshape(lb + 1, la + 1) for x in d1.pair_matrices(p))
            M2, A2, B2 = (x.reshape(la + 1, lb + 1) for x in d2.pair_matrices(p))
            assert np.array_equal(M1, M2.T) and np.array_equal(A1, B2.T) and np.array_equal(B1, A2.T)


# --------------------------------------------------- host-level + legacy surface --
def test_host_level_fill_batch_and_chunking(ctx):
    import os
    sc = S.make_scoring({"preset": "default"})
    batch = W.ragged(300, seed=4, max_len=120)
    M, A, B, off, status = ctx.fill_batch(batch, sc, 0)
    osc = oracle_scoring_of(sc)
    for p in range(0, 300, 7):
        rc, oM, oA, oB = O.oracle_fill(osc, batch.seq_a(p), batch.seq_b(p), 0)
        o, n = int(off[p]), oM.size
        assert np.array_equal(M[o:o + n], oM) and np.array_equal(A[o:o + n], oA) and np.array_equal(B[o:o + n], oB)
    # tiny chunk budget -> many chunks, same bytes
    with S.Context(0) as small:
        small.set_option("chunk_bytes", 1 << 20)
        M2, A2, B2, _, _ = small.fill_batch(batch, sc, 0)
    assert np.array_equal(M, M2) and np.array_equal(A, A2) and np.array_equal(B, B2)


@pytest.mark.parametrize("where", ["device", "host", "device-three-matrices"])
def test_nw_batch_strings_match_oracle_and_golden(ctx, where, opts):
    """End-to-end NW: GPU fill + traceback on the device (default: for plain scorings the fill writes only a byte of
    directions per cell, sa_fill_dirs.hip; "device-three-matrices": the three matrices and the walkers that re-derive
    every step from them) or on the host from the copied-back matrices (option traceback=host); identical strings."""
    if where == "device-three-matrices":
        opts(nw_dirs=0)
    else:
        opts(traceback=where)
    cfg = load("configs.json")["C2_related"]
    sc = S.make_scoring(cfg["scoring"])
    batch = W.make(cfg["gen"], cfg["n"], cfg["kwargs"])
    res = ctx.nw_batch(batch, sc)
    for p, g in enumerate(cfg["pairs"]):
        assert res[p] == (g["score"], g["result_a"].encode(), g["result_b"].encode())
    # every flag combination (inside the parity domain) + ragged incl. empty sequences, vs oracle
    for idx, flags in enumerate(itertools.product([0, 1], repeat=5)):
        spec = {"init": [1, -6 if (flags[2] and flags[3]) else -2, -4, -1, *flags, idx & 1],
                "wildcards": [["N", -1]] if idx % 3 == 0 else []}
        sc = S.make_scoring(spec)
        batch = W.ragged(24, seed=idx + 10, max_len=70, lower_frac=0.2, extra=b"N" if spec["wildcards"] else b"")
        res = ctx.nw_batch(batch, sc)
        osc = oracle_scoring_of(sc)
        for p in range(batch.n_pairs):
            rc, s, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and res[p] == (s, ra, rb)


@pytest.mark.parametrize("dirs", [1, 0], ids=["directions", "three-matrices"])
@pytest.mark.parametrize("n_sub", [2, 5, 16])
def test_nw_batch_pipelined_subbatches(ctx, opts, n_sub, dirs):
    """seqalign_nw_batch with a chunk cut into sub-batches that overlap fill / traceback / copies on two streams
    (sa_batch.hip: nw_chunk; by default only for large chunks, forced here): same strings and scores as
    the reference's needleman_wunsch_align (src/needleman_wunsch.c:53-145) -- golden C2 pairs, a ragged batch with
    empty sequences and sub-batch cuts inside runs of tiny pairs -- and an unknown character pair inside one
    sub-batch is still reported (alignment_scoring.c:178-181)."""
    opts(subbatches=n_sub, nw_dirs=dirs)
    cfg = load("configs.json")["C2_related"]
    sc = S.make_scoring(cfg["scoring"])
    res = ctx.nw_batch(W.make(cfg["gen"], cfg["n"], cfg["kwargs"]), sc)
    for p, g in enumerate(cfg["pairs"]):
        assert res[p] == (g["score"], g["result_a"].encode(), g["result_b"].encode())
    osc = oracle_scoring_of(sc)
    r = W.ragged(400, seed=300 + n_sub, max_len=180, lower_frac=0.1)
    pairs = [(b"", b""), (b"A", b""), (b"", b"C")] * 5 + [(r.seq_a(p), r.seq_b(p)) for p in range(r.n_pairs)] + [(b"G", b"G")] * 7
    batch = W.from_pairs(pairs)
    res = ctx.nw_batch(batch, sc)
    for p in range(batch.n_pairs):
        rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
        assert rc == 0 and res[p] == (s_, ra, rb), (n_sub, p)
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    bad = W.from_pairs([(b"ACGT", b"ACGT")] * 40 + [(b"ACGT", b"AXGT")] + [(b"ACGT", b"ACGT")] * 40)
    with pytest.raises(S.SeqAlignError) as err:
        ctx.nw_batch(bad, hyb)
    assert err.value.code == S.E_UNKNOWN_PAIR


@pytest.mark.parametrize("max_hits", [1, 4])
def test_sw_batch_reports_an_unknown_character_pair(ctx, max_hits):
    """A character pair without a score (use_match_mismatch = 0: the reference exits there, alignment_scoring.c:178-181) fails the
    local call with SEQALIGN_E_UNKNOWN_PAIR whatever path the other pairs would take -- small and large (packed-fill sized)
    batches, best hit and several hits."""
    hyb = S.make_scoring({"preset": "DNA_hybridization"})
    good = (b"ACGTACGTAC" * 6, b"TTACGTACGTACGA" * 5)
    for n in (9, 2500):
        pairs = [good] * n
        assert all(len(h) >= 1 for h in ctx.sw_batch(W.from_pairs(pairs), hyb, 5, max_hits=max_hits))
        pairs[n // 2] = (good[0], good[1][:20] + b"X" + good[1][21:])
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_batch(W.from_pairs(pairs), hyb, 5, max_hits=max_hits)
        assert err.value.code == S.E_UNKNOWN_PAIR


@pytest.mark.parametrize("max_len", [40, 100, 180, 250, 300, 380, 500, 511, 512, 513, 700, 767, 768, 1000, 1023, 1024, 1025])
def test_direction_byte_paths_every_width(ctx, max_len):
    """The direction-byte fills (sa_fill_dirs.hip) in every columns-per-lane instantiation and on both sides of their
    limits (SW: 511 is the widest row they take, 512 / 513 / 700 go through the three matrices; NW, round 5: rows up to 1 024
    columns -- 12 and 16 columns per lane -- and the three matrices beyond; no seam anywhere): seqalign_nw_batch strings and seqalign_sw_batch hit lists (max_hits 1 and 6) against the oracle, default
    options, plain scorings incl. a substitution table (BLOSUM62 -> the LDS-table instantiation) and a wildcard."""
    rng = W.Rng(4000 + max_len)

    def rand(n, alpha):
        return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""

    for spec, alpha in (({"preset": "default"}, b"ACGT"), ({"preset": "BLOSUM62"}, b"ARNDCQEGHILKMFPSTWYV"),
                        ({"init": [2, -3, -5, -2, 0, 0, 0, 0, 0, 0], "wildcards": [["N", 0]]}, b"ACGTN")):
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        pairs = []
        for k in range(10):
            la = max_len if k < 3 else int(1 + rng.below(max_len, 1)[0])
            lb = int(1 + rng.below(90, 1)[0]) if k % 2 else int(20 + rng.below(60, 1)[0])
            a = rand(la, alpha)
            b = a[la // 3: la // 3 + lb] if (k % 3 == 0 and la >= 3) else rand(lb, alpha)   # planted / unrelated
            pairs.append((a, b or rand(5, alpha)))
        pairs += [(b"", rand(7, alpha)), (rand(max_len, alpha), b"")]
        batch = W.from_pairs(pairs)
        res = ctx.nw_batch(batch, sc)
        for p in range(batch.n_pairs):
            rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and res[p] == (s_, ra, rb), (max_len, spec, "nw", p)
        thr = 12 if "preset" in spec and spec["preset"] == "BLOSUM62" else 8
        for max_hits in (1, 6):
            got = ctx.sw_batch(batch, sc, thr, max_hits=max_hits)
            for p in range(batch.n_pairs):
                rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), thr, max_hits)
                assert rc == 0 and got[p] == want, (max_len, spec, "sw", max_hits, p)


@pytest.mark.parametrize("shape", [(0, 0), (0, 7), (7, 0), (1, 1), (1, 9), (9, 1), (5, 3), (63, 64), (64, 33), (127, 70), (128, 128), (150, 150),
                                   (191, 40), (192, 25), (255, 130), (300, 60), (383, 20), (450, 30), (511, 45),
                                   (512, 40), (600, 33), (767, 21), (768, 30), (1000, 25), (1023, 18)])
def test_nw_batch_two_pairs_per_wave(ctx, opts, shape):
    """Batches whose pairs all have one shape take the packed direction fill (sa_fill_dirs_x2.hip: two pairs per wave,
    int16 halves; option pack16 -- 2: also for chunks below the 1 025 pairs from which it pays): strings and scores equal the oracle's (needleman_wunsch.c:53-145) and the one-pair
    kernel's (pack16 = 0) for every columns-per-lane instantiation, odd and even pair counts (the last wave of an odd
    launch holds one pair), unrelated and related sequences, gap_open = 0, sub-batches cut at odd pairs, substitution
    tables -- and a scoring whose scores could leave int16 is NOT packed (same results through the 32-bit kernel)."""
    la, lb = shape
    rng = W.Rng(9100 + 7 * la + lb)
    dna = np.frombuffer(b"ACGT", np.uint8)
    for n, spec, n_sub in ((1, {"preset": "default"}, 0), (2, {"init": [2, -3, 0, -2, 0, 0, 0, 0, 0, 1], "wildcards": []}, 0),
                           (37, {"preset": "default"}, 3), (64, {"init": [3, -1, -7, -1, 0, 0, 0, 0, 0, 0], "wildcards": []}, 0),
                           (21, {"init": [40, -60, -90, -30, 0, 0, 0, 0, 0, 0], "wildcards": []}, 2)):
        a = dna[rng.below(4, n * la).astype(np.int64)].reshape(n, la)
        b = dna[rng.below(4, n * lb).astype(np.int64)].reshape(n, lb)
        k = min(la, lb)
        keep = rng.unit(n * k).reshape(n, k) < 0.8          # half of the pairs related: b = a with substitutions
        b[: n // 2, :k] = np.where(keep[: n // 2], a[: n // 2, :k], b[: n // 2, :k])
        batch = W._fixed_batch(a, b)
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        opts(pack16=2, subbatches=n_sub)
        packed = ctx.nw_batch(batch, sc)
        opts(pack16=0, subbatches=n_sub)
        plain = ctx.nw_batch(batch, sc)
        assert packed == plain, (shape, n, spec)
        for p in range(n):
            rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and packed[p] == (s_, ra, rb), (shape, n, spec, p)
    # scorings with a substitution table (the K x K table as int16 in LDS, two 16-bit reads per packed cell): BLOSUM62 on
    # protein, and a wildcard (class 0 x class 0 with different characters takes the mismatch score)
    for n, spec, alpha in ((33, {"preset": "BLOSUM62"}, b"ARNDCQEGHILKMFPSTWYVBZX"), (18, {"preset": "PAM70"}, b"ARNDCQEGHILKMFPSTWYV"),
                           (25, {"init": [2, -3, -5, -2, 0, 0, 0, 0, 0, 0], "wildcards": [["N", 0]]}, b"ACGTN")):
        al = np.frombuffer(alpha, np.uint8)
        a = al[rng.below(len(al), n * la).astype(np.int64)].reshape(n, la)
        b = al[rng.below(len(al), n * lb).astype(np.int64)].reshape(n, lb)
        k = min(la, lb)
        keep = rng.unit(n * k).reshape(n, k) < 0.7
        b[: n // 2, :k] = np.where(keep[: n // 2], a[: n // 2, :k], b[: n // 2, :k])
        batch = W._fixed_batch(a, b)
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        opts(pack16=2, subbatches=0)
        packed = ctx.nw_batch(batch, sc)
        opts(pack16=0, subbatches=0)
        assert packed == ctx.nw_batch(batch, sc), (shape, n, spec)
        for p in range(n):
            rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and packed[p] == (s_, ra, rb), (shape, n, spec, p)


@pytest.mark.parametrize("n_sub", [0, 3])
def test_nw_batch_mostly_one_shape(ctx, opts, n_sub):
    """A chunk whose pairs are MOSTLY of one shape (reads of one length, some trimmed), on the default route (moves come home):
    the pairs that find a partner of their shape go through the packed kernel two per wave and the others through the one-pair
    kernel, side by side in one grid per sub-batch with the list of its pairs (sa_batch.hip: nw_chunk, pair_up_shapes;
    SaFillParams::pair_list).  Strings and scores equal the oracle's and the one-pair path's, with the
    odd ones (other lengths, empty sequences) scattered through the batch, for one and for several sub-batches, at a
    size where the packed kernel is chosen by itself (2 600 pairs) and forced on a small batch."""
    rng = W.Rng(4242 + n_sub)
    sc = S.make_scoring({"preset": "default"})
    osc = oracle_scoring_of(sc)

    def rand(n):
        return bytes(b"ACGT"[i] for i in rng.below(4, n)) if n else b""

    for n, pk in ((2600, 1), (90, 2)):
        pairs = []
        for k in range(n):
            if k % 7 == 3:      # the odd ones
                la, lb = int(rng.below(160, 1)[0]), int(rng.below(160, 1)[0])
            else:
                la, lb = 100, 100
            a = rand(la)
            b = (a[: lb] + rand(max(0, lb - la))) if k % 2 else rand(lb)
            pairs.append((a, b))
        batch = W.from_pairs(pairs)
        opts(pack16=pk, subbatches=n_sub)
        got = ctx.nw_batch(batch, sc)
        opts(pack16=0, subbatches=n_sub)
        assert got == ctx.nw_batch(batch, sc), (n, pk)
        for p in range(0, n, 1 if n < 200 else 23):
            rc, s_, ra, rb = O.oracle_nw(osc, pairs[p][0], pairs[p][1])
            assert rc == 0 and got[p] == (s_, ra, rb), (n, pk, p)


@pytest.mark.parametrize("shape", [(0, 0), (0, 6), (6, 0), (1, 1), (9, 2), (5, 40), (63, 64), (64, 33), (127, 70), (150, 200), (191, 40),
                                   (192, 25), (255, 90), (300, 60), (383, 20), (450, 30), (511, 45),
                                   (512, 40), (600, 50), (768, 30), (1000, 40), (1023, 25)])   # (beyond 511: the best-hit fill only)
def test_sw_batch_two_pairs_per_wave(ctx, opts, shape):
    """The SW multi-hit path on batches whose pairs all have one shape: the packed fill of match_scores + directions
    (sa_fill_dirs_x2.hip: fill_dirs_x2_kernel, two pairs per wave in int16 halves; the sweep and the hit walks read what
    it wrote).  Hit lists (score, positions, strings, order: smith_waterman.c:71-86, 137-277) equal the oracle's and the
    one-pair kernel's (pack16 = 0) for every columns-per-lane instantiation, odd and even pair counts, planted repeats
    (several hits per pair, ties), low thresholds, max_hits 1 / 3 / unlimited."""
    la, lb = shape
    rng = W.Rng(9500 + 7 * la + lb)
    dna = np.frombuffer(b"ACGT", np.uint8)
    for n, spec, thr, max_hits in ((1, {"preset": "default"}, 3, 1 << 20), (2, {"init": [2, -3, 0, -2, 0, 0, 0, 0, 0, 1], "wildcards": []}, 4, 3),
                                   (37, {"preset": "default"}, 5, 1 << 20), (64, {"init": [3, -1, -7, -1, 0, 0, 0, 0, 0, 0], "wildcards": []}, 9, 1),
                                   (21, {"init": [1, -1, -2, 0, 0, 0, 0, 0, 0, 0], "wildcards": []}, 2, 6)):
        a = dna[rng.below(4, n * la).astype(np.int64)].reshape(n, la)
        b = dna[rng.below(4, n * lb).astype(np.int64)].reshape(n, lb)
        k = min(la, lb)
        if k >= 8:          # half of the pairs: a piece of a planted in b, twice where it fits (repeats -> several hits, ties)
            piece = max(4, k // 3)
            for r in range(n // 2):
                src = int(rng.below(la - piece + 1, 1)[0])
                for dst in {int(rng.below(lb - piece + 1, 1)[0]), int(rng.below(lb - piece + 1, 1)[0])}:
                    b[r, dst:dst + piece] = a[r, src:src + piece]
        batch = W._fixed_batch(a, b)
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        opts(pack16=2)
        packed = ctx.sw_batch(batch, sc, thr, max_hits=max_hits, hit_cap=1 << 16)
        opts(pack16=0)
        plain = ctx.sw_batch(batch, sc, thr, max_hits=max_hits, hit_cap=1 << 16)
        assert packed == plain, (shape, n, spec)
        for p in range(n):
            rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), thr, max_hits)
            assert rc == 0 and packed[p] == want, (shape, n, spec, p)
    # substitution tables (BLOSUM62 on protein, a wildcard): best hit (fill_sw_best_x2_kernel) and several hits
    for n, spec, alpha, thr in ((29, {"preset": "BLOSUM62"}, b"ARNDCQEGHILKMFPSTWYVBZX", 14),
                                (20, {"init": [2, -3, -5, -2, 0, 0, 0, 0, 0, 0], "wildcards": [["N", 0]]}, b"ACGTN", 6)):
        al = np.frombuffer(alpha, np.uint8)
        a = al[rng.below(len(al), n * la).astype(np.int64)].reshape(n, la)
        b = al[rng.below(len(al), n * lb).astype(np.int64)].reshape(n, lb)
        k = min(la, lb)
        if k >= 8:
            piece = max(4, k // 2)
            for r in range(n // 2):
                src, dst = int(rng.below(la - piece + 1, 1)[0]), int(rng.below(lb - piece + 1, 1)[0])
                b[r, dst:dst + piece] = a[r, src:src + piece]
        batch = W._fixed_batch(a, b)
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        for max_hits in (1, 5):
            opts(pack16=2)
            packed = ctx.sw_batch(batch, sc, thr, max_hits=max_hits, hit_cap=1 << 16)
            opts(pack16=0)
            assert packed == ctx.sw_batch(batch, sc, thr, max_hits=max_hits, hit_cap=1 << 16), (shape, n, spec, max_hits)
            for p in range(n):
                rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), thr, max_hits)
                assert rc == 0 and packed[p] == want, (shape, n, spec, max_hits, p)


@pytest.mark.parametrize("dirs", [1, 0], ids=["directions", "three-matrices"])
def test_nw_batch_in_several_chunks(ctx, dirs):
    """seqalign_nw_batch on a batch that does not fit one chunk (tiny chunk budget): per-chunk scratch (descriptor block,
    direction bytes or matrices, string slots, pinned staging) is reused chunk after chunk; results equal the one-chunk
    call's and the oracle's."""
    sc = S.make_scoring({"preset": "default"})
    batch = W.dna_nw_150(150, seed=83, length=140, related=True)
    one = ctx.nw_batch(batch, sc)
    with S.Context(0) as small:
        small.set_option("chunk_bytes", 6 << 20)     # ~25 pairs per chunk
        small.set_option("nw_dirs", dirs)
        small.set_option("subbatches", 3)
        many = small.nw_batch(batch, sc)
    assert one == many
    osc = oracle_scoring_of(sc)
    for p in range(0, batch.n_pairs, 11):
        rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
        assert rc == 0 and one[p] == (s_, ra, rb), p


def test_context_options(ctx):
    """seqalign_ctx_set_option: unknown keys and out-of-range values are refused (nothing changes), options are
    per context, and the environment is read once, when a context is created."""
    with pytest.raises(S.SeqAlignError) as err:
        ctx.set_option("no_such_option", 1)
    assert err.value.code == S.E_ARG
    for key, val in (("kernel", "fastest"), ("traceback", "nowhere"), ("sweep_strip", 100), ("wpb", 3), ("chunk_bytes", 17)):
        with pytest.raises(S.SeqAlignError):
            ctx.set_option(key, val)
    sc = S.make_scoring({"preset": "default"})
    batch = W.dna_nw_150(64, seed=3, related=True)
    want = ctx.nw_batch(batch, sc)
    os.environ["SEQALIGN_TRACEBACK"] = "host"
    try:
        with S.Context(0) as other:          # picks "host" up at creation ...
            os.environ["SEQALIGN_TRACEBACK"] = "nonsense"   # ... and never looks again
            assert other.nw_batch(batch, sc) == want
            assert ctx.nw_batch(batch, sc) == want
    finally:
        del os.environ["SEQALIGN_TRACEBACK"]
    for k, v in S.OPTION_DEFAULTS.items():   # every documented key is accepted with its default
        ctx.set_option(k, v)


@pytest.mark.parametrize("walker", ["lane", "wave", "directions", "directions-lane", "directions-wave", "directions-wave-1", "directions-wave-4", "directions-wave-8"])
def test_device_traceback_walkers_agree_with_oracle(ctx, walker, opts):
    """The device walkers -- one lane per pair from the three matrices in HBM, one wave per pair from 16x16 LDS tiles
    of them, and the ones that follow the fill's direction bytes (sa_fill_dirs.hip; plain scorings, rows <= 512
    columns, everything else falls back) -- on pairs that cross many tiles, hug the borders and end in long gap runs."""
    if walker == "directions":
        opts(nw_dirs=1, sweep_dirs=1)
    elif walker.startswith("directions-"):      # one lane per walk from HBM / one wave per walk from 64 x 64-byte LDS tiles
        # (round 6: -4 / -8: four / eight walks per wave in lockstep, option walk_group)
        opts(nw_dirs=1, sweep_dirs=1, trace_kernel=walker.split("-")[1], walk_group=int((walker.split("-") + ["0"])[2]))
    else:
        opts(trace_kernel=walker, nw_dirs=0, sweep_dirs=0)
    pairs = [(b"ACGT" * 40, b"ACGT" * 40), (b"A" * 100, b"A" * 17), (b"C" * 5, b"G" * 90), (b"ACGTTGCA" * 9, b"TTTT" + b"ACGTTGCA" * 7),
             (b"G", b"G"), (b"", b"ACGT"), (b"ACGT", b"")]
    r = W.ragged(40, seed=91, max_len=260, lower_frac=0.1)
    pairs += [(r.seq_a(p), r.seq_b(p)) for p in range(r.n_pairs)]
    rel = W.dna_nw_150(6, seed=92, length=700, related=True)
    pairs += [(rel.seq_a(p), rel.seq_b(p)[:650 + 7 * p]) for p in range(rel.n_pairs)]
    batch = W.from_pairs(pairs)
    for spec in ({"preset": "default"}, {"init": [1, -2, -4, -1, 1, 1, 0, 0, 0, 0]}, {"init": [2, -3, -5, -2, 0, 0, 0, 1, 0, 0]}):
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        res = ctx.nw_batch(batch, sc)
        for p in range(batch.n_pairs):
            rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and res[p] == (s_, ra, rb), (walker, spec, p)
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    osc = oracle_scoring_of(sc)
    got = ctx.sw_batch(batch, sc, 6, max_hits=1)
    for p in range(batch.n_pairs):
        rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), 6, 1)
        assert rc == 0 and got[p] == want, (walker, p)


@pytest.mark.parametrize("max_hits,where", [(5, "device"), (16, "device"), (1, "device"), (1, "host"), (5, "host"),
                                            (40, "device")])
def test_sw_batch_hits_match_oracle(ctx, max_hits, where, opts):
    """max_hits=1: fill + reduction + traceback of the best hit on the device;
    max_hits<=16: candidates sorted and enumerated on the device (one lane per pair);
    larger / option traceback=host: candidates + matrices go back, host enumerates."""
    opts(traceback=where)
    for spec, gen, kw, thr in (
            ({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}, W.dna_sw_read_vs_ref, dict(seed=21, read_len=60, ref_len=300), 24),
            ({"preset": "BLOSUM62"}, W.protein_sw_300, dict(seed=22, length=120), 24),
            ({"init": [1, -2, -4, -1, 0, 0, 1, 1, 0, 1]}, W.dna_nw_150, dict(seed=23, length=40, related=True), 3),
            # free start/end gaps + asymmetric mutations, as in the reference's examples/sw_example.c:30-46
            ({"init": [1, -2, -4, -1, 1, 1, 0, 0, 0, 0], "mutations": [["a", "c", -2], ["c", "a", -1]]},
             W.dna_nw_150, dict(seed=24, length=70, related=True), 4)):
        sc = S.make_scoring(spec)
        batch = gen(24, **kw)
        got = ctx.sw_batch(batch, sc, thr, max_hits=max_hits)
        osc = oracle_scoring_of(sc)
        for p in range(batch.n_pairs):
            rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), thr, max_hits)
            assert rc == 0 and got[p] == want, (spec, p)


@pytest.mark.parametrize("name", ["C3", "C4"])
@pytest.mark.parametrize("where", ["device", "host", "device-three-matrices"])
def test_sw_batch_hit_lists_at_config_size(ctx, name, where, opts):
    """seqalign_sw_batch at the BASELINE dimensions (150x1000 DNA / 300x300 BLOSUM62, --minscore 60): the ordered
    hit lists of 64 seeded pairs, max_hits 1 and unlimited, against the committed ORACLE-DERIVED lists
    (tests/golden/sw_hits_oracle.json -- the reference's smith_waterman.c cannot be built here) and a live
    oracle run.  "device" takes the direction-byte path (sa_fill_dirs.hip: both configs are in its domain),
    "device-three-matrices" round 2's.  Reference: src/smith_waterman.c:137-277."""
    if where == "device-three-matrices":
        opts(sweep_dirs=0)
    else:
        opts(traceback=where)
    g = load("sw_hits_oracle.json")[name]
    sc = S.make_scoring({"preset": "BLOSUM62"} if g["scoring"] == "BLOSUM62" else g["scoring"])
    osc = oracle_scoring_of(sc)
    batch = W.make(g["gen"], g["n"], g["kwargs"])
    for max_hits in (1, 1 << 20):
        got = ctx.sw_batch(batch, sc, g["min_score"], max_hits=max_hits)
        for p in range(batch.n_pairs):
            want = [dict(score=h[0], pos_a=h[1], pos_b=h[2], len_a=h[3], len_b=h[4], a=h[5], b=h[6])
                    for h in g["hits"][p][:max_hits]]
            assert got[p] == want, (name, max_hits, p)
            if p % 8 == 0:
                rc, live = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), g["min_score"], max_hits)
                assert rc == 0 and live == want


def _refwalk_sections():
    g = load("sw_hits_refwalk.json")
    for name in ("C3", "C4", "C3_low", "C4_low"):
        e = g[name]
        batch = W.make(e["gen"], e["of"], e["kwargs"])
        yield name, e["scoring"], batch.slice(0, e["n"]), e["min_score"], e["hits"]
    for k, r in enumerate(g["repeats"]):
        yield f"repeats[{k}]", r["scoring"], W.from_pairs([(a.encode(), b.encode()) for a, b in r["pairs"]]), r["min_score"], r["hits"]


@pytest.mark.parametrize("where", ["device", "device-three-matrices", "device-first-sweep-form"])
def test_sw_batch_equals_the_reference_walked_hit_lists(ctx, where, opts):
    """seqalign_sw_batch against tests/golden/sw_hits_refwalk.json -- hit lists in which every score, every
    matrix cell and every traceback step was computed by the COMPILED REFERENCE (aligner_align + alignment_reverse_move; candidate
    order and visited mask of smith_waterman.c:71-86,137-277 restated in Python, tests/orclib.py: ref_sw_hits), not by our own C
    restatement: all hits >= 60 of the 64 C3 / C4 pairs, 24-58 hits per pair at threshold 15 (walks abandoned at marked cells,
    marks left behind), and tandem repeats under twelve scorings with gap flags / wildcards / free end gaps (ties on score AND
    column).  Unlimited max_hits and a cut-off of 3; the direction-byte path, the three-matrix path, the sweep's first form."""
    if where == "device-three-matrices":
        opts(sweep_dirs=0)
    elif where == "device-first-sweep-form":
        opts(sweep_ev=0)
    total = 0
    for label, spec, batch, thr, rows in _refwalk_sections():
        sc = S.make_scoring(spec)
        for max_hits in (1 << 20, 3):
            got = ctx.sw_batch(batch, sc, thr, max_hits=max_hits, hit_cap=1 << 16)
            for p in range(batch.n_pairs):
                want = [dict(score=h[0], pos_a=h[1], pos_b=h[2], len_a=h[3], len_b=h[4], a=h[5], b=h[6]) for h in rows[p][:max_hits]]
                assert got[p] == want, (label, where, max_hits, p, len(got[p]), len(want))
                total += len(want)
    assert total > 3000


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_sw_batch_full_size_hit_list_properties(ctx, name):
    """seqalign_sw_batch with up to 4 hits per pair on the FULL config (10 000 x 150x1000 DNA / 4 000 x 300x300
    BLOSUM62), through properties that do not need the oracle's minutes: (1) hit 0 of every pair is the hit the
    best-hit path (max_hits = 1: fill's best cell + one traceback) reports; (2) every hit's two strings re-score to
    its score under the scoring (substitutions + affine gaps) and are the sequences' own characters at pos / len;
    (3) a pair's hits come in the reference's order (score desc, then end column asc, then end row asc) and never
    share a cell (smith_waterman.c:187-199: a walk that meets a marked cell is no hit); (4) a strided sample equals
    the oracle's sequential enumeration."""
    cfg = FULL[name]
    sc = S.make_scoring(cfg["scoring"])
    osc = oracle_scoring_of(sc)
    batch = cfg["gen"](cfg["n"], **cfg["kwargs"])
    thr = W.default_minscore(sc.match, int(batch.len_a[0]), int(batch.len_b[0]))
    n = batch.n_pairs
    multi = ctx.sw_batch(batch, sc, thr, max_hits=4, hit_cap=4 * n + 8)
    best = ctx.sw_batch(batch, sc, thr, max_hits=1, hit_cap=n + 8)
    table = np.zeros((128, 128), np.int64)
    for x in range(32, 127):
        for y in range(32, 127):
            s_, m_ = C.c_int(0), C.c_int(0)
            if O.oracle().orc_scoring_lookup(C.byref(osc), C.c_char(bytes([x])), C.c_char(bytes([y])), C.byref(s_), C.byref(m_)) == 0:
                table[x, y] = s_.value
    go, ge = osc.gap_open, osc.gap_extend
    assert sum(len(h) for h in multi) >= n // 2
    for p in range(n):
        assert multi[p][:1] == best[p], (name, p)
        a, b = batch.seq_a(p), batch.seq_b(p)
        cells, prev = set(), None
        for h in multi[p]:
            sa_, sb_ = h["a"].encode(), h["b"].encode()
            assert sa_.replace(b"-", b"") == a[h["pos_a"]:h["pos_a"] + h["len_a"]]
            assert sb_.replace(b"-", b"") == b[h["pos_b"]:h["pos_b"] + h["len_b"]]
            score, x, y, in_gap = 0, h["pos_a"], h["pos_b"], 0
            for ca, cb in zip(sa_, sb_):
                if ca == 45 or cb == 45:
                    which = 1 if ca == 45 else 2
                    score += ge + (go if in_gap != which else 0)
                    in_gap = which
                    x, y = x + (cb == 45), y + (ca == 45)
                else:
                    score += int(table[ca, cb]); in_gap = 0
                    x, y = x + 1, y + 1
                assert (x, y) not in cells, (name, p)
                cells.add((x, y))
            assert score == h["score"] >= thr, (name, p, score, h["score"])
            key = (-h["score"], h["pos_a"] + h["len_a"], h["pos_b"] + h["len_b"])
            assert prev is None or prev < key, (name, p)
            prev = key
    for p in range(0, n, max(1, n // 12)):
        rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), thr, 4)
        assert rc == 0 and multi[p] == want, (name, p)


@pytest.mark.parametrize("pad_cells", [32, 1])
def test_workgroup_stream_kernel_long_rows(ctx, pad_cells):
    """sa_fill_wgstream.hip: rows of 513 .. 4 096 columns split over 4 or 8 waves of one
    workgroup -- every columns-per-lane / wave-count instantiation, both ends of its range,
    NW / SW / protein table, pairs starting at arbitrary 4-byte offsets (pad_cells=1)."""
    import torch
    rng = W.Rng(404)

    def rand(n, alpha=b"ACGT"):
        return bytes(alpha[i] for i in rng.below(len(alpha), n))

    lens = [512, 767, 768, 1023, 1024, 1279, 1280, 1535, 1536, 2047, 2048, 2559, 2560, 3071, 3072, 4095]
    for spec, is_sw, alpha in (({"preset": "default"}, 0, b"ACGT"), ({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}, 1, b"ACGT"),
                               ({"preset": "BLOSUM62"}, 1, b"ARNDCQEGHILKMFPSTWYV")):
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        h = ctx.upload_scoring(sc, is_sw)
        for group in (lens[:2], lens[2:4], lens[4:7], lens[7:10], lens[10:13], lens[13:]):   # one launch per family
            pairs = [(rand(la, alpha), rand(40 + (la % 37), alpha)) for la in group] + [(rand(group[0] - 300, alpha), b"")]
            batch = W.from_pairs(pairs)
            db = S.DeviceBatch(batch, 0, pad_cells=pad_cells, placement="packed")
            db.M.fill_(-7); db.A.fill_(-7); db.B.fill_(-7)
            db.fill(ctx, h, S.KERNEL_WGSTREAM)
            torch.cuda.synchronize()
            assert_pairs_match_oracle(db, batch, osc, is_sw, range(batch.n_pairs), tag=f"wgstream {spec} {group}")
        ctx.release_scoring(h)


def test_workgroup_stream_kernel_general_scorings(ctx):
    """sa_fill_wgstream.hip, GENERAL instantiations: free end gaps, no gaps in a / b, no
    mismatches, gap_open > 0, a missing pair (status = first failing cell) -- on long rows."""
    import torch
    rng = W.Rng(505)

    def rand(n, alpha=b"ACGT"):
        return bytes(alpha[i] for i in rng.below(len(alpha), n))

    groups = ([767, 1023], [1536, 2047], [2560, 4095])
    specs = [({"init": [1, -2, -4, -1, 0, 1, 0, 0, 0, 0]}, 0), ({"init": [1, -2, -4, -1, 1, 1, 0, 0, 0, 0]}, 0),
             ({"init": [1, -2, -4, -1, 0, 0, 1, 0, 0, 0]}, 0), ({"init": [1, -2, -4, -1, 0, 0, 0, 1, 0, 0]}, 0),
             ({"init": [1, -2, -4, -1, 0, 1, 0, 1, 0, 0]}, 1), ({"init": [2, -2, -2, -1, 0, 0, 0, 0, 1, 0]}, 1),
             ({"init": [1, -2, 2, -3, 0, 0, 0, 0, 0, 0]}, 0),
             ({"init": [1, -2, -4, -1, 0, 1, 0, 0, 0, 0], "wildcards": [["N", -1]]}, 0)]
    for spec, is_sw in specs:
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        h = ctx.upload_scoring(sc, is_sw)
        for group in groups:
            alpha = b"ACGTN" if spec.get("wildcards") else b"ACGT"
            pairs = [(rand(la, alpha), rand(23 + la % 11, alpha)) for la in group]
            batch = W.from_pairs(pairs)
            db = S.DeviceBatch(batch, 0, pad_cells=1, placement="packed")
            db.M.fill_(-7); db.A.fill_(-7); db.B.fill_(-7)
            db.fill(ctx, h, S.KERNEL_WGSTREAM)
            torch.cuda.synchronize()
            assert_pairs_match_oracle(db, batch, osc, is_sw, range(batch.n_pairs), tag=f"wgstream general {spec} {group}")
            assert (db.status.cpu().numpy() == -1).all()
        ctx.release_scoring(h)
    # a pair without a score: the first failing cell in row-major order, as the other kernels report it
    sc = S.make_scoring({"preset": "DNA_hybridization"})
    h = ctx.upload_scoring(sc, 0)
    a = bytearray(rand(1500)); a[700] = ord("N"); a[20] = ord("N")
    b = bytearray(rand(30)); b[3] = ord("X")
    batch = W.from_pairs([(bytes(a), rand(30)), (rand(1500), bytes(b)), (rand(900), rand(12))])
    got = {}
    for kid in (S.KERNEL_ROWSCAN, S.KERNEL_WGSTREAM):
        db = S.DeviceBatch(batch, 0, placement="packed")
        db.fill(ctx, h, kid)
        torch.cuda.synchronize()
        got[kid] = db.status.cpu().numpy().view(np.uint64).copy()
    assert np.array_equal(got[S.KERNEL_ROWSCAN], got[S.KERNEL_WGSTREAM])
    assert got[S.KERNEL_WGSTREAM][0] == 1 * 1501 + 21 and got[S.KERNEL_WGSTREAM][1] == 4 * 1501 + 1
    assert got[S.KERNEL_WGSTREAM][2] == S.STATUS_OK
    ctx.release_scoring(h)


def test_sw_best_hit_on_long_rows(ctx):
    """sw_batch(max_hits=1) with the long sequence as seq_a: the workgroup kernel reports the best cell
    itself (<= 2 048 columns; beyond that the separate reduction runs) -- hits equal the oracle's."""
    rng = W.Rng(606)

    def rand(n):
        return bytes(b"ACGT"[i] for i in rng.below(4, n))

    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    osc = oracle_scoring_of(sc)
    pairs = []
    for la in (600, 900, 1024, 1500, 2047, 2600):
        ref = rand(la)
        cut = int(rng.below(la - 80, 1)[0])
        read = ref[cut:cut + 60] + rand(5) + ref[cut + 65:cut + 80]
        pairs.append((ref, read))
    pairs += [(b"ACGT" * 300, b"ACGT" * 10), (rand(1300), b"")]         # ties across many columns; an empty read
    for group in (pairs[:2] * 70, pairs[2:5] * 50, pairs[5:] * 50):      # >= 128 pairs: AUTO takes the workgroup kernel
        batch = W.from_pairs(group)
        got = ctx.sw_batch(batch, sc, 20, max_hits=1)
        for p in range(0, batch.n_pairs, 7):
            rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), 20, 1)
            assert rc == 0 and got[p] == want, p


def test_multi_context_calls_equal_single_context(ctx):
    """seqalign_*_batch_multi: the pairs split over several contexts (here three on the one
    device of the test box; one per GPU on a node) -- results identical to one context."""
    peers = [S.Context(0), S.Context(0)]
    try:
        sc = S.make_scoring({"preset": "default"})
        batch = W.ragged(101, seed=55, max_len=120, lower_frac=0.1)     # 101: uneven ranges
        assert ctx.nw_batch(batch, sc, peers=peers) == ctx.nw_batch(batch, sc)
        one = ctx.fill_batch(batch, sc, 0)
        many = ctx.fill_batch(batch, sc, 0, peers=peers)
        for x, y in zip(one, many):
            assert np.array_equal(x, y)
        sw = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
        sb = W.dna_sw_read_vs_ref(50, seed=56, read_len=40, ref_len=200)
        for max_hits in (1, 5, 40):
            assert ctx.sw_batch(sb, sw, 6, max_hits=max_hits, peers=peers) == ctx.sw_batch(sb, sw, 6, max_hits=max_hits)
        # ranges are cut at equal cells (sa_multi.hip: shard_edges): second half 10x longer sequences
        r1, r2 = W.ragged(40, seed=57, max_len=30), W.dna_nw_150(40, seed=58, length=300, related=True)
        lop = W.from_pairs([(r1.seq_a(p), r1.seq_b(p)) for p in range(40)] + [(r2.seq_a(p), r2.seq_b(p)) for p in range(40)])
        assert ctx.nw_batch(lop, sc, peers=peers) == ctx.nw_batch(lop, sc)
        assert ctx.sw_batch(lop, sw, 8, max_hits=3, peers=peers) == ctx.sw_batch(lop, sw, 8, max_hits=3)
        tiny = W.from_pairs([(b"ACGT", b"AGGT")])                        # fewer pairs than contexts
        assert ctx.nw_batch(tiny, sc, peers=peers) == ctx.nw_batch(tiny, sc)
        # ... and the multi-context results against the ORACLE directly, not only against one context:
        # matrices, global alignments, local hit lists of the ragged / lopsided batches above
        osc, osw = oracle_scoring_of(sc), oracle_scoring_of(sw)
        M, A, B, mat_off, status = many
        res = ctx.nw_batch(lop, sc, peers=peers)
        hits = ctx.sw_batch(lop, sw, 8, max_hits=3, peers=peers)
        for p in range(0, batch.n_pairs, 7):
            rc, oM, oA, oB = O.oracle_fill(osc, batch.seq_a(p), batch.seq_b(p), 0)
            o = int(mat_off[p])
            assert rc == 0 and np.array_equal(M[o:o + oM.size], oM) and np.array_equal(A[o:o + oA.size], oA) and np.array_equal(B[o:o + oB.size], oB), p
        for p in range(lop.n_pairs):
            rc, s_, ra, rb = O.oracle_nw(osc, lop.seq_a(p), lop.seq_b(p))
            assert rc == 0 and res[p] == (s_, ra, rb), p
            rc, want = O.oracle_sw(osw, lop.seq_a(p), lop.seq_b(p), 8, 3)
            assert rc == 0 and hits[p] == want, p
    finally:
        for c in peers:
            c.close()


def test_arena_allocator(ctx):
    """seqalign_arenas_alloc: three 4 KiB-aligned device buffers the fill accepts; small requests are plain
    allocations and not probed (quality < 0); large ones are built from hipMemCreate chunks, the third arena
    chosen by the write probe -- the walk is reported (seqalign_arenas_info) and ends at the target or takes the
    best candidate; with arena_scan_gib = 0 they are three hipMallocs.  Every byte of a placed arena is writable
    and readable (chunks mapped back to back), and the memory comes back on free."""
    import torch
    lib = S.lib()
    torch.cuda.empty_cache()      # (torch's cached blocks are not the library's: the checks below make it cache gigabytes)
    free0 = torch.cuda.mem_get_info(0)[0]
    for nbytes, placed in ((1 << 20, False), (300 << 20, True), ((1 << 30) + 12345 * 4096, True)):
        ptrs = (C.c_void_p * 3)()
        q = C.c_float(0.0)
        assert lib.seqalign_arenas_alloc(ctx._h, C.c_uint64(nbytes), ptrs, C.byref(q)) == 0
        assert all(p and p % 4096 == 0 for p in ptrs) and len({int(p) for p in ptrs}) == 3
        info = S.ArenaInfo()
        assert lib.seqalign_arenas_info(ctx._h, ptrs, C.byref(info)) == 0
        d = info.as_dict()
        assert (q.value > 0.3) if placed else (q.value < 0)
        assert d["vmm"] == placed and abs(d["quality"] - q.value) < 1e-3
        if placed:
            assert 1 <= d["tries"] <= 96 and d["second_walk_from"] <= d["tries"] and d["chunk_mib"] == 512 and len(d["try_quality"]) == d["tries"]
            assert d["quality"] >= d["target"] - 0.05 or d["tries"] > 1      # below target only after looking further
            assert max(d["try_quality"]) >= d["quality"] - 0.08               # the kept candidate is (about) the best seen
            n = nbytes // 4
            for k, p_ in enumerate(ptrs):   # first / last words and every chunk seam
                t = torch.as_tensor(S._RawDeviceInts(p_, n), device="cuda:0")
                t.fill_(k + 1)
                idx = torch.tensor([0, n - 1] + [j for j in range((512 << 20) // 4 - 1, n, (512 << 20) // 4) for j in (j, min(j + 1, n - 1))],
                                   device="cuda:0")
                assert int(t.sum().item()) == (k + 1) * n and bool((t[idx] == k + 1).all())
                del t
        assert lib.seqalign_arenas_free(ctx._h, ptrs) == 0
        assert not any(ptrs)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    # round 5: up to arena_keep_gib of a walk's unused chunks (and the freed arenas' own) stay with the process -- the chunk pool
    held = ctx.pool_trim()
    assert held % (512 << 20) == 0 and held <= int(ctx.get_option("arena_keep_gib")) << 30
    assert torch.cuda.mem_get_info(0)[0] >= free0 - held - (64 << 20)
    assert ctx.pool_trim(0) == 0
    assert torch.cuda.mem_get_info(0)[0] >= free0 - (64 << 20)      # spacer chunks and arenas all returned
    with S.Context(0) as plain:
        plain.set_option("arena_scan_gib", 0)
        ptrs = (C.c_void_p * 3)()
        assert lib.seqalign_arenas_alloc(plain._h, C.c_uint64(300 << 20), ptrs, None) == 0
        info = S.ArenaInfo()
        assert lib.seqalign_arenas_info(plain._h, ptrs, C.byref(info)) == 0 and not info.vmm and info.tries == 0
        assert lib.seqalign_arenas_free(plain._h, ptrs) == 0
        bogus = (C.c_void_p * 3)(4096, 8192, 12288)
        assert lib.seqalign_arenas_free(plain._h, bogus) == S.E_ARG
    # a batch on library-placed arenas and one on a packed allocation give the same bytes
    sc = S.make_scoring({"preset": "default"})
    batch = W.dna_nw_150(3000, seed=5)
    h = ctx.upload_scoring(sc, 0)
    a = S.DeviceBatch(batch, 0, placement="spread", ctx=ctx)
    b = S.DeviceBatch(batch, 0, placement="packed")
    for db in (a, b):
        db.M.fill_(-7); db.A.fill_(-7); db.B.fill_(-7)
        db.fill(ctx, h, S.KERNEL_AUTO)
    torch.cuda.synchronize()
    assert torch.equal(a.M, b.M) and torch.equal(a.A, b.A) and torch.equal(a.B, b.B)
    ctx.release_scoring(h)


SWEEP_VARIANTS = {
    "default": {},                                    # plain scorings, rows <= 512 columns: match_scores + direction bytes
                                                      # (sa_fill_dirs.hip); else three matrices, form by sequence length
    "first-form": {"sweep_ev": 0},                    # the direction-byte sweep with keys and states in separate registers (round 3's;
                                                      # default since round 4: a walk as one word key << 2 | state, one min3 per cell)
    "three-matrices": {"sweep_dirs": 0},              # the three-matrix path everywhere (round 2's)
    "segments-64": {"sweep_cpl": 1},                  # 64-column segments: several per row where the walks spread out
    "segments-256": {"sweep_cpl": 4},
    "strips": {"sweep_mode": "strips", "sweep_strip": 64},   # one wave per 64-column strip of a pair
    "box-pass": {"kernel": "rowscan"},                # a fill that cannot report the candidates' box and rows itself
}


@pytest.fixture(params=list(SWEEP_VARIANTS))
def sweep_variant(request, opts):
    opts(**SWEEP_VARIANTS[request.param])
    return request.param


def test_sw_sweep_enumeration(ctx, sweep_variant):
    """sa_sw_sweep.hip: every hit of a pair from one reverse sweep over the matrices, against the sequential
    procedure (oracle) -- plume-heavy pairs (planted homologs, low thresholds), tandem repeats (ties, many hits),
    the max_hits cut, BLOSUM62, scores in the tens of thousands (wide key fields), empty sequences."""
    rng = W.Rng(909)

    def rand(n, alpha=b"ACGT"):
        return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""

    dna = W.dna_sw_read_vs_ref(20, seed=71, read_len=100, ref_len=400)
    pairs = [(dna.seq_a(p), dna.seq_b(p)) for p in range(dna.n_pairs)]
    for k in range(16):
        unit = rand(4 + k % 6)
        pairs.append((unit * (5 + k % 7) + rand(k % 9), rand(k % 5) + unit * (8 + k % 11)))
    pairs += [(b"ACGT" * 40, b"ACGT" * 70), (b"A" * 120, b"A" * 150), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A")]
    batch = W.from_pairs(pairs)
    for spec, thr in (({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}, 10), ({"init": [1, -1, -3, -1, 0, 0, 0, 0, 0, 0]}, 4),
                      ({"init": [3, -3, -4, -2, 0, 0, 0, 0, 1, 0]}, 9), ({"init": [1, 0, 0, 0, 0, 0, 0, 0, 0, 0]}, 3)):
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        for max_hits in (2, 7, 16, 1 << 20):
            got = ctx.sw_batch(batch, sc, thr, max_hits=max_hits, hit_cap=400000)
            for p in range(batch.n_pairs):
                rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), thr, max_hits)
                assert rc == 0 and got[p] == want, (sweep_variant, spec, max_hits, p)
    prot = W.protein_sw_300(10, seed=72, length=150)
    sc = S.make_scoring({"preset": "BLOSUM62"})
    osc = oracle_scoring_of(sc)
    got = ctx.sw_batch(prot, sc, 25, max_hits=1 << 20)
    for p in range(prot.n_pairs):
        rc, want = O.oracle_sw(osc, prot.seq_a(p), prot.seq_b(p), 25)
        assert rc == 0 and got[p] == want, (sweep_variant, "BLOSUM62", p)
    sc = S.make_scoring({"init": [30000, -20000, -25000, -5000, 0, 0, 0, 0, 0, 0]})
    osc = oracle_scoring_of(sc)
    got = ctx.sw_batch(dna, sc, 250000, max_hits=5)
    for p in range(dna.n_pairs):
        rc, want = O.oracle_sw(osc, dna.seq_a(p), dna.seq_b(p), 250000, 5)
        assert rc == 0 and got[p] == want, (sweep_variant, "large scores", p)


@pytest.mark.parametrize("mode", ["default", "pair", "strips", "wgstream-fill"])
def test_sw_sweep_wide_pairs_and_many_hits(ctx, mode, opts):
    """Wide rows (600 .. 2 500 columns: 1 200+ take a fill that cannot report the candidates' box and rows itself;
    one wave per pair with the winners of two rows in LDS, or one wave per 256-column strip -- the default for few
    pairs and beyond 2 048 columns) and pairs with hundreds of hits (more than the 64 the sweep ranks itself: ordered
    by the host) -- against the oracle."""
    if mode == "wgstream-fill":      # the workgroup-per-pair fill reports the candidates' box and rows itself
        opts(kernel="wgstream", sweep_mode="pair")
    elif mode != "default":
        opts(sweep_mode=mode)
    rng = W.Rng(1717)

    def rand(n, alpha=b"ACGT"):
        return bytes(alpha[i] for i in rng.below(len(alpha), n)) if n else b""

    def planted(la, lb):
        ref = rand(lb)
        cut = int(rng.below(max(1, lb - min(la, lb) + 1), 1)[0])
        return (ref[cut:cut + la] + rand(max(0, la - (lb - cut))))[:la], ref

    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    osc = oracle_scoring_of(sc)
    wide = W.from_pairs([planted(la, 70 + la % 90) for la in (600, 1023, 1024, 1500, 2500)] +
                        [(rand(700), rand(90)), (b"ACGT" * 200, b"ACGT" * 30), planted(90, 70)])
    for thr, max_hits in ((30, 4), (8, 1 << 20)):
        got = ctx.sw_batch(wide, sc, thr, max_hits=max_hits, hit_cap=100000)
        for p in range(wide.n_pairs):
            rc, want = O.oracle_sw(osc, wide.seq_a(p), wide.seq_b(p), thr, max_hits)
            assert rc == 0 and got[p] == want, ("wide", mode, thr, p)
    # two long, closely related sequences: the plume of the one hit covers most of a 1 300 x 1 170 matrix (every
    # strip and nearly every row has walks on it)
    a = bytearray(rand(1300))
    b = bytearray(a[:1170])
    for i in range(0, len(b), 23):
        b[i] = b"ACGT"[(b"ACGT".index(b[i]) + 1) % 4]
    square = W.from_pairs([(bytes(a), bytes(b)), (bytes(b[:700]), bytes(a[100:1200]))])
    got = ctx.sw_batch(square, sc, 300, max_hits=5, hit_cap=1000)
    for p in range(square.n_pairs):
        rc, want = O.oracle_sw(osc, square.seq_a(p), square.seq_b(p), 300, 5)
        assert rc == 0 and got[p] == want, ("square", mode, p)
    many = W.from_pairs([(rand(300), rand(300)) for _ in range(3)] + [(b"ACGTTGCA" * 30, b"TGCAACGT" * 40)])
    for max_hits in (70, 1 << 20):
        got = ctx.sw_batch(many, sc, 4, max_hits=max_hits, hit_cap=400000)
        for p in range(many.n_pairs):
            rc, want = O.oracle_sw(osc, many.seq_a(p), many.seq_b(p), 4, max_hits)
            assert rc == 0 and got[p] == want, ("many hits", mode, max_hits, p)
        assert max(len(h) for h in got) > 64


def test_sw_batch_output_capacity_is_respected(ctx):
    """seqalign_sw_batch with too few hit slots: SEQALIGN_E_NOMEM, nothing written past the caller's capacity (the
    hits that fit are delivered, in order)."""
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    batch = W.from_pairs([(b"ACGTTGCA" * 12, b"TGCAACGT" * 30)] * 3)
    full = ctx.sw_batch(batch, sc, 8, max_hits=6)
    assert all(len(h) == 6 for h in full)
    for max_hits in (1, 6):
        with pytest.raises(S.SeqAlignError) as err:
            ctx.sw_batch(batch, sc, 8, max_hits=max_hits, hit_cap=2 if max_hits == 1 else 7)
        assert err.value.code == 4   # SEQALIGN_E_NOMEM


@pytest.mark.parametrize("nw_moves", [1, 0])
def test_sw_batch_out_of_room_delivers_what_fits(ctx, nw_moves):
    """the best-hit path with the moves walkers returned SEQALIGN_E_NOMEM before expanding the hits of the chunk that
    did fit, the string path after -- the same call gave different *n_hits by an internal option.  Both deliver the fitting
    prefix (in pair order, equal to the uncapped call's first hits), then SEQALIGN_E_NOMEM."""
    import ctypes as C
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    batch = W.dna_sw_read_vs_ref(40, seed=7, read_len=60, ref_len=200)
    with S.Context(0) as c:
        c.set_option("nw_moves", nw_moves)
        full = c.sw_batch(batch, sc, 20, max_hits=1)
        assert sum(len(h) for h in full) >= 30
        hit_cap = 11
        hits = (S.SwHit * hit_cap)()
        str_cap = hit_cap * (60 + 200 + 2)
        out_a, out_b = np.zeros(str_cap, np.uint8), np.zeros(str_cap, np.uint8)
        n_hits = C.c_uint64(0)
        ms = np.full(batch.n_pairs, 20, np.int32)
        d = S.batch_desc(batch)
        rc = S.lib().seqalign_sw_batch(c._h, C.byref(d), C.byref(sc), S._ptr(ms), C.c_uint32(1), hits, C.c_uint64(hit_cap),
                                       C.byref(n_hits), S._ptr(out_a), S._ptr(out_b), C.c_uint64(str_cap))
        assert rc == 4 and n_hits.value == hit_cap          # SEQALIGN_E_NOMEM, and every slot used
        flat = [(p, h) for p, hs in enumerate(full) for h in hs]
        for k in range(hit_cap):
            h, (p, want) = hits[k], flat[k]
            got = dict(score=h.score, pos_a=h.pos_a, pos_b=h.pos_b, len_a=h.len_a, len_b=h.len_b,
                       a=out_a[h.str_off:h.str_off + h.length].tobytes().decode(), b=out_b[h.str_off:h.str_off + h.length].tobytes().decode())
            assert h.pair == p and got == want, (k, p)


# ---- seqalign_sw_batch's four ways home under a capacity: 130 pairs of one shape are three delivery blocks of 64, 64 and 2 pairs
# (path name, max_hits, extra options, whether the walks send home moves)
SW_ROOM_PATHS = [("best hit on moves", 1, {}, True), ("best hit on strings", 1, {"nw_moves": 0}, False),
                 ("one-trip", 4, {}, True), ("three-trip", 9, {}, False)]   # (the one-trip form stops at 8 hits per pair)
SW_ROOM_THRESHOLD = 20   # (more than 65 of the 130 pairs have a hit at 20: asserted below)
SW_ROOM_SENTINEL = 0xEE


@pytest.fixture(scope="module")
def sw_room_batch():
    return W.dna_sw_read_vs_ref(130, seed=7, read_len=60, ref_len=200)


def _sw_room_call(c, batch, sc, max_hits, hit_cap, str_cap, cigar):
    """One raw seqalign_sw_batch (or _cigar, format M) call into sentinel-filled buffers: (rc, the delivered hits as
    (record fields without str_off, text a, text b), bytes used per hit, the output arrays, the hit array)."""
    hits = (S.SwHit * (hit_cap + 1))()
    C.memset(hits, SW_ROOM_SENTINEL, C.sizeof(hits))
    out_a, out_b = np.full(str_cap + 1, SW_ROOM_SENTINEL, np.uint8), np.full(str_cap + 1, SW_ROOM_SENTINEL, np.uint8)
    n_hits = C.c_uint64(0)
    ms = np.full(batch.n_pairs, SW_ROOM_THRESHOLD, np.int32)
    d = S.batch_desc(batch)
    if cigar:
        rc = S.lib().seqalign_sw_batch_cigar(c._h, C.byref(d), C.byref(sc), S._ptr(ms), C.c_uint32(max_hits), C.c_int(1), hits,
                                             C.c_uint64(hit_cap), C.byref(n_hits), S._ptr(out_a), C.c_uint64(str_cap))
    else:
        rc = S.lib().seqalign_sw_batch(c._h, C.byref(d), C.byref(sc), S._ptr(ms), C.c_uint32(max_hits), hits, C.c_uint64(hit_cap),
                                       C.byref(n_hits), S._ptr(out_a), S._ptr(out_b), C.c_uint64(str_cap))
    got, used = [], 0
    for k in range(n_hits.value):
        h = hits[k]
        assert h.str_off == used, (k, h.str_off, used)   # the hits lie back to back
        if cigar:
            end = int(h.str_off)
            while out_a[end]:
                end += 1
            text = (out_a[h.str_off:end].tobytes(), b"")
            used = end + 1
        else:
            text = (out_a[h.str_off:h.str_off + h.length].tobytes(), out_b[h.str_off:h.str_off + h.length].tobytes())
            assert out_a[h.str_off + h.length] == 0 and out_b[h.str_off + h.length] == 0, k
            used += h.length + 1
        got.append(((h.pair, h.score, h.pos_a, h.pos_b, h.len_a, h.len_b, h.length), text, used - int(h.str_off)))
    # nothing behind the used part was touched, in the strings and in the records
    assert (out_a[used:] == SW_ROOM_SENTINEL).all() and (cigar or (out_b[used:] == SW_ROOM_SENTINEL).all()), (hit_cap, str_cap, used)
    assert bytes(hits[hit_cap]) == bytes([SW_ROOM_SENTINEL]) * C.sizeof(S.SwHit), (hit_cap, str_cap)
    return rc, got


def _sw_room_check(c, batch, sc, max_hits, moves, cigar, caps_of):
    ample_hits, ample_str = 130 * max_hits, 130 * max_hits * (60 + 200 + 2)
    rc, full = _sw_room_call(c, batch, sc, max_hits, ample_hits, ample_str, cigar)
    ran = c.last_call()
    assert any(k.startswith("walk_moves_") for k in ran) == moves, ran
    assert rc == 0 and len(full) > 65, (rc, len(full))
    assert [f[0][0] for f in full] == sorted(f[0][0] for f in full)          # pair order
    H, need = len(full), np.cumsum([0] + [f[2] for f in full])               # need[h]: the bytes of the first h hits
    for hit_cap, str_cap in caps_of(H, need, ample_hits, ample_str):
        fits = max(h for h in range(H + 1) if h <= hit_cap and need[h] <= str_cap)
        rc, got = _sw_room_call(c, batch, sc, max_hits, hit_cap, str_cap, cigar)
        assert any(k.startswith("walk_moves_") for k in c.last_call()) == moves, c.last_call()
        assert rc == (0 if fits == H else 4), (hit_cap, str_cap, rc)          # SEQALIGN_E_NOMEM after what fits
        assert len(got) == fits, (hit_cap, str_cap, len(got), fits)
        assert got == full[:fits], (hit_cap, str_cap)


@pytest.mark.parametrize("path", SW_ROOM_PATHS, ids=[p[0].replace(" ", "-") for p in SW_ROOM_PATHS])
def test_sw_batch_room_prefix_on_every_path(sw_room_batch, path):
    """Every way seqalign_sw_batch brings hits home -- best hit on moves, best hit on strings, the one-trip and the three-trip
    multi-hit forms -- delivers, under any hit_cap / str_cap, exactly the longest prefix of the uncapped call's hits (pair order)
    whose count and bytes (length + 1 per hit) fit: record for record, string for string, nothing written behind the used part,
    then SEQALIGN_E_NOMEM; with room for everything the call returns 0 and the uncapped result.  The caps sit on the edges of
    the delivery blocks of 64 pairs."""
    name, max_hits, options, moves = path
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    with S.Context(0) as c:
        c.set_option("pack16", 2)   # the packed fills, and with them the moves forms, at this size
        for k, v in options.items():
            c.set_option(k, v)

        def caps_of(H, need, ample_hits, ample_str):
            caps = [(hc, ample_str) for hc in (0, 1, 63, 64, 65, H - 1)]
            for h in (1, 64, 65):
                caps += [(ample_hits, int(need[h])), (ample_hits, int(need[h]) - 1)]
            return caps + [(H, int(need[H]))]
        _sw_room_check(c, sw_room_batch, sc, max_hits, moves, False, caps_of)


@pytest.mark.parametrize("path", [SW_ROOM_PATHS[0], SW_ROOM_PATHS[2]], ids=["best-hit-on-moves", "one-trip"])
def test_sw_batch_cigar_room_prefix_on_moves_paths(sw_room_batch, path):
    """... and seqalign_sw_batch_cigar (format M) on the two moves forms, where a hit's bytes are its CIGAR's length + 1 counted
    from the planes: hit_cap 65, and the bytes of 65 hits minus one."""
    name, max_hits, options, moves = path
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    with S.Context(0) as c:
        c.set_option("pack16", 2)
        _sw_room_check(c, sw_room_batch, sc, max_hits, moves, True,
                       lambda H, need, ample_hits, ample_str: [(65, ample_str), (ample_hits, int(need[65]) - 1)])


def test_sw_batch_multi_hit_in_several_chunks(ctx):
    """seqalign_sw_batch(max_hits > 1) on a batch that does not fit one chunk (tiny chunk budget): the per-chunk
    scratch (hit keys, walker lists, string slots) is reused chunk after chunk; hits equal the one-chunk call's."""
    sc = S.make_scoring({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]})
    batch = W.dna_sw_read_vs_ref(120, seed=73, read_len=80, ref_len=300)
    one = ctx.sw_batch(batch, sc, 16, max_hits=6)
    with S.Context(0) as small:
        small.set_option("chunk_bytes", 6 << 20)     # ~30 pairs per chunk
        many = small.sw_batch(batch, sc, 16, max_hits=6)
    assert one == many
    osc = oracle_scoring_of(sc)
    for p in range(0, batch.n_pairs, 9):
        rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), 16, 6)
        assert rc == 0 and one[p] == want, p


def test_sw_enumeration_repeats_and_ties(ctx, sweep_variant):
    """Device multi-hit enumeration on inputs built to stress its order rules: tandem
    repeats (many equal-score candidates: column-ascending, then index-ascending ties),
    long walks, many hits per pair and the max_hits cut must reproduce the sequential
    reference procedure."""
    rng = W.Rng(77)

    def rand(n):
        return bytes(b"ACGT"[i] for i in rng.below(4, n)) if n else b""

    pairs = []
    for k in range(40):
        unit = rand(3 + k % 7)
        a = unit * (4 + k % 9) + rand(k % 13)
        b = rand(k % 11) + unit * (6 + k % 17) + unit[::-1] * (k % 5)
        pairs.append((a, b))
    pairs += [(b"ACGT" * 30, b"ACGT" * 80), (b"A" * 90, b"A" * 200), (b"", b"ACGT"), (b"ACGTTGCA" * 12, b"TGCAACGT" * 30)]
    batch = W.from_pairs(pairs)
    for spec, thr in (({"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}, 8), ({"init": [1, -1, -3, -1, 0, 0, 0, 0, 0, 0]}, 3),
                      ({"init": [3, -3, -4, -2, 0, 0, 0, 0, 1, 0]}, 12)):
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        for max_hits in (1, 3, 16):   # 1: the best cell comes from the fill kernel itself
            got = ctx.sw_batch(batch, sc, thr, max_hits=max_hits)
            for p in range(batch.n_pairs):
                rc, want = O.oracle_sw(osc, batch.seq_a(p), batch.seq_b(p), thr, max_hits)
                assert rc == 0 and got[p] == want, (sweep_variant, spec, max_hits, p)
            assert max(len(h) for h in got) == max_hits   # the cut is exercised


def test_legacy_api_known_answers(ctx):
    """The reference's own tests (tests.c) replayed against OUR library through the
    reference-shaped API: needleman_wunsch_align / smith_waterman_fetch."""
    lib = S.lib()
    kat = load("kat.json")
    nw = C.c_void_p(lib.needleman_wunsch_new())
    res = C.c_void_p(lib.alignment_create(C.c_size_t(256)))
    for v in kat["nw"]:                      # same aligner re-used, like tests.c:133-163
        sc = S.make_scoring(v["scoring"])
        lib.needleman_wunsch_align(v["a"].encode(), v["b"].encode(), C.byref(sc), nw, res)
        r = O.Alignment.from_address(res.value)
        assert (C.string_at(r.result_a).decode(), C.string_at(r.result_b).decode()) == (v["result_a"], v["result_b"])
        if "score" in v:
            assert r.score == v["score"]
    lib.needleman_wunsch_free(nw)
    for v in kat["sw"]:
        sc = S.make_scoring(v["scoring"])
        sw = C.c_void_p(lib.smith_waterman_new())
        a, b = v["a"].encode(), v["b"].encode()
        lib.smith_waterman_align(a, b, C.byref(sc), sw)
        for want in v["hits"]:
            assert lib.smith_waterman_fetch(sw, res) == 1
            r = O.Alignment.from_address(res.value)
            assert [C.string_at(r.result_a).decode(), C.string_at(r.result_b).decode()] == want
        # a re-used sw_aligner_t gives the hits of a fresh one
        lib.smith_waterman_align(a, b, C.byref(sc), sw)
        assert lib.smith_waterman_fetch(sw, res) == 1
        r = O.Alignment.from_address(res.value)
        assert [C.string_at(r.result_a).decode(), C.string_at(r.result_b).decode()] == v["hits"][0]
        lib.smith_waterman_free(sw)
    lib.alignment_free(res)


def test_legacy_sw_fetch_matches_oracle_hit_lists(ctx):
    lib = S.lib()
    spec = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}
    sc, osc = S.make_scoring(spec), O.build_scoring(spec, "oracle")
    batch = W.dna_sw_read_vs_ref(6, seed=31, read_len=50, ref_len=200)
    sw = C.c_void_p(lib.smith_waterman_new())
    res = C.c_void_p(lib.alignment_create(C.c_size_t(16)))
    for p in range(batch.n_pairs):
        a, b = batch.seq_a(p), batch.seq_b(p)
        lib.smith_waterman_align2(a, b, C.c_size_t(len(a)), C.c_size_t(len(b)), C.byref(sc), sw)
        rc, want = O.oracle_sw(osc, a, b, 0, 12)
        for h in want:
            assert lib.smith_waterman_fetch(sw, res) == 1
            r = O.Alignment.from_address(res.value)
            assert (r.score, r.pos_a, r.pos_b, r.len_a, r.len_b, C.string_at(r.result_a).decode(),
                    C.string_at(r.result_b).decode()) == (h["score"], h["pos_a"], h["pos_b"], h["len_a"],
                                                         h["len_b"], h["a"], h["b"])
    lib.smith_waterman_free(sw)
    lib.alignment_free(res)


def test_legacy_api_one_aligner_per_thread_runs_in_parallel(ctx):
    """The reference's aligner_align mutates only its own aligner_t (src/alignment.c:170-202), so one aligner per thread
    runs in parallel (SURVEY 8b "Threading").  Here every calling thread gets its own device context, and callers that
    are in the library at the same time share launches (sa_device.hip: combine_and_run -- a launch takes ~50 us whatever
    it carries).  A plain-C program written the way a seq-align user would write it (examples/legacy_threads.c: pthreads,
    one nw_aligner_t per thread, needleman_wunsch_align) must get the single-thread answers in every thread and well
    over three times the single-thread pairs per second with 8 threads (asserted: 3.2x, on a box whose host is busy with this test process's own threads) (rounds 1-2: one context behind one mutex, 1x;
    one launch per call and thread: 3.3-4.0x; measured with shared launches: 4.8x at 8 threads, 7.1x at 16 -- 73 k and
    105 k pairs/s against 15 k).  (Python threads cannot show it: the interpreter's own per-call work is serial.)"""
    import subprocess
    exe = Path(S.__file__).resolve().parents[2] / "bin" / "legacy_threads"
    assert exe.exists(), "seq-align_amd/bin/legacy_threads is built by `make` (__graft_entry__.build)"
    best = None
    for attempt in range(3):      # (a shared box: take the best of three runs)
        out = subprocess.run([str(exe), "8", "40"], capture_output=True, text=True, timeout=300)   # 8 threads x 1 920 pairs
        assert out.returncode == 0, out.stdout + out.stderr
        res = json.loads(out.stdout.strip().splitlines()[-1])
        assert res["identical"] is True
        best = res if best is None or res["speedup"] > best["speedup"] else best
        if best["speedup"] > 3.2:
            break
    assert best["speedup"] > 3.2, best


def test_legacy_api_concurrent_callers_with_different_scorings(ctx):
    """Concurrent callers of the reference-shaped API share launches (sa_device.hip: combine_and_run), but only callers
    with the SAME scoring and algorithm: six threads -- three scorings, NW and SW mixed, pairs of different sizes, each
    thread its own aligner -- must all get what the oracle gets, call after call (ctypes releases the GIL during a call,
    so the threads really are in the library together)."""
    import threading
    lib = S.lib()
    specs = [{"preset": "default"}, {"init": [2, -3, -5, -2, 0, 0, 0, 0, 0, 0]}, {"init": [3, -1, 0, -1, 0, 0, 0, 0, 0, 1]}]
    rng = W.Rng(7717)

    def rand(n):
        return bytes(b"ACGT"[i] for i in rng.below(4, n))

    jobs = []
    for t in range(6):
        spec, is_sw = specs[t % 3], t >= 3
        osc = oracle_scoring_of(S.make_scoring(spec))
        pairs = []
        for k in range(40):
            a = rand(int(8 + rng.below(120, 1)[0]))
            b = a[3:] if k % 3 == 0 else rand(int(8 + rng.below(120, 1)[0]))
            if is_sw:
                rc, hits = O.oracle_sw(osc, a, b, 0, 1)
                want = (hits[0]["score"], hits[0]["a"], hits[0]["b"]) if hits else None
            else:
                rc, s_, ra, rb = O.oracle_nw(osc, a, b)
                want = (s_, ra.decode(), rb.decode())
            pairs.append((a, b, want))
        jobs.append((spec, is_sw, pairs))
    errors = []

    def work(spec, is_sw, pairs):
        try:
            sc = S.make_scoring(spec)
            res = C.c_void_p(lib.alignment_create(C.c_size_t(512)))
            al = C.c_void_p(lib.smith_waterman_new() if is_sw else lib.needleman_wunsch_new())
            for rep in range(5):
                for a, b, want in pairs:
                    if is_sw:
                        lib.smith_waterman_align2(a, b, C.c_size_t(len(a)), C.c_size_t(len(b)), C.byref(sc), al)
                        got = None
                        if lib.smith_waterman_fetch(al, res) == 1:
                            r = O.Alignment.from_address(res.value)
                            got = (r.score, C.string_at(r.result_a).decode(), C.string_at(r.result_b).decode())
                    else:
                        lib.needleman_wunsch_align2(a, b, C.c_size_t(len(a)), C.c_size_t(len(b)), C.byref(sc), al, res)
                        r = O.Alignment.from_address(res.value)
                        got = (r.score, C.string_at(r.result_a).decode(), C.string_at(r.result_b).decode())
                    if got != want:
                        errors.append((spec, is_sw, a, b, got, want))
                        return
            (lib.smith_waterman_free if is_sw else lib.needleman_wunsch_free)(al)
            lib.alignment_free(res)
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=j) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors[:2]


def test_legacy_api_sees_scoring_edits_between_calls(ctx):
    """The per-pair API keeps the flattened scoring on the device while the caller's
    scoring_t is unchanged; an edit through the same pointer must be picked up."""
    lib = S.lib()
    sc = S.make_scoring({"preset": "default"})
    nw = C.c_void_p(lib.needleman_wunsch_new())
    res = C.c_void_p(lib.alignment_create(C.c_size_t(64)))
    a, b = b"ACGTTGCAAC", b"ACGATGCTAC"

    def run():
        lib.needleman_wunsch_align(a, b, C.byref(sc), nw, res)
        r = O.Alignment.from_address(res.value)
        return r.score, C.string_at(r.result_a), C.string_at(r.result_b)

    for step in range(3):
        rc, s, ra, rb = O.oracle_nw(oracle_scoring_of(sc), a, b)
        assert rc == 0 and run() == (s, ra, rb) and run() == (s, ra, rb)
        if step == 0:
            lib.scoring_add_mutation(C.byref(sc), C.c_char(b"t"), C.c_char(b"a"), C.c_int(3))
        else:
            sc.gap_extend = -2
            sc.min_penalty = min(sc.min_penalty, sc.gap_open + sc.gap_extend)
    lib.alignment_free(res)
    lib.needleman_wunsch_free(nw)


@pytest.mark.parametrize("kernel", KERNELS, ids=KID)
def test_dense_packing_and_odd_arena_alignment(ctx, kernel):
    """Pairs packed back to back (pad_cells=1: every 4-byte alignment of a pair's
    first cell, neighbours share 1 KiB blocks) -- the stream kernel's partial first /
    last blocks must not touch a neighbour's cells; and arenas that are NOT congruent
    mod 4 KiB, where the stream kernel must hand over to the row-store kernel."""
    import torch
    sc = S.make_scoring({"preset": "default"})
    osc = oracle_scoring_of(sc)
    batch = W.ragged(200, seed=77, max_len=150)
    h = ctx.upload_scoring(sc, 0)
    db = S.DeviceBatch(batch, 0, pad_cells=1)
    for t in (db.M, db.A, db.B):
        t.fill_(0x5A5A5A5A)
    db.fill(ctx, h, kernel)
    torch.cuda.synchronize()
    assert_pairs_match_oracle(db, batch, osc, 0, range(batch.n_pairs), tag=f"dense {KID(kernel)}")
    # skewed arenas: rebuild the descriptor with A shifted by 5 ints, B by 300
    total = db.total_cells
    raw = torch.full((3 * total + 4096,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    M, A, B = raw[0:total], raw[total + 5:2 * total + 5], raw[2 * total + 300:3 * total + 300]
    db.M, db.A, db.B = M, A, B
    db.desc.match_scores, db.desc.gap_a_scores, db.desc.gap_b_scores = M.data_ptr(), A.data_ptr(), B.data_ptr()
    db.fill(ctx, h, kernel)
    torch.cuda.synchronize()
    assert_pairs_match_oracle(db, batch, osc, 0, range(batch.n_pairs), tag=f"skewed {KID(kernel)}")
    # nothing outside the three arenas was written
    assert int((raw[total:total + 5] != 0x5A5A5A5A).sum()) == 0
    assert int((raw[2 * total + 5:2 * total + 300] != 0x5A5A5A5A).sum()) == 0
    assert int((raw[3 * total + 300:] != 0x5A5A5A5A).sum()) == 0
    ctx.release_scoring(h)


def test_randomised_scorings_differential(ctx):
    """A few hundred random (scoring, batch) combinations through the default
    kernel choice, NW and SW: penalties, all five flags, case sensitivity,
    wildcards and asymmetric mutations drawn from a seeded stream."""
    rng = W.Rng(20260928)
    checked = 0
    for trial in range(60):
        v = rng.below(1 << 20, 12).astype(int)
        flags = [int(v[0] >> k) & 1 for k in range(5)]
        match, mismatch = int(v[1] % 6), -int(v[2] % 7)
        go, ge = -int(v[3] % 12), -int(v[4] % 4)
        if flags[2] and flags[3]:
            mismatch = min(mismatch, go + ge)
        spec = {"init": [match, mismatch, go, ge, *flags, int(v[5] & 1)], "wildcards": [], "mutations": []}
        if v[6] & 1:
            spec["wildcards"].append(["N", int(v[6] % 5) - 2])
        if v[7] & 1:
            spec["mutations"] += [["a", "g", int(v[7] % 7) - 3], ["g", "a", int(v[8] % 7) - 3], ["T", "c", 2]]
        sc = S.make_scoring(spec)
        osc = oracle_scoring_of(sc)
        batch = W.ragged(16, seed=int(v[9]), max_len=int(20 + v[10] % 200), lower_frac=0.25,
                         extra=b"N" if spec["wildcards"] else b"")
        for is_sw in (0, 1):
            if not is_sw and min(osc.gap_open + osc.gap_extend, osc.gap_extend) < -abs(osc.min_penalty):
                continue
            db = device_fill(ctx, batch, sc, is_sw, S.KERNEL_AUTO)
            assert_pairs_match_oracle(db, batch, osc, is_sw, range(batch.n_pairs), tag=f"trial {trial} {spec}")
            checked += batch.n_pairs
    assert checked > 1500


# ---- seqalign_nw_batch's pipeline (sa_batch.hip): sub-batches, groups, streams, staging or in place, per result form ------------

import nwbatchlib as NB  # noqa: E402

NW_ROUTES = {"default": {}, "zero_copy=0": {"zero_copy": 0}, "zero_copy=1": {"zero_copy": 1}, "zero_copy=2": {"zero_copy": 2},
             "zero_copy=3": {"zero_copy": 3}, "zero_copy=auto": {"zero_copy": "auto"}, "nw_moves=0": {"nw_moves": 0}, "nw_dirs=0": {"nw_dirs": 0}}
NW_PIPELINE_SHAPES = list(itertools.product((0, 2, 5), (0, 1), (1, 4), (0, 2)))   # subbatches x walk_overlap x upload_slices x pack16


@pytest.fixture(scope="module")
def small_ragged(ctx):
    """The 1 300-pair batch (packed and unpacked host blocks), the default route's results and the oracle's: computed once."""
    batch, pairs = NB.half_packed_ragged()
    sc = S.make_scoring({"preset": "default"})
    osc = oracle_scoring_of(sc)
    want = []
    for a, b in pairs:
        rc, s_, ra, rb = O.oracle_nw(osc, a, b)
        assert rc == 0
        want.append((s_, ra, rb))
    base = ctx.nw_batch(batch, sc)
    assert set(ctx.last_call()) == {"fill_nw_dirs", "walk_moves_tile"}, ctx.last_call()
    bad = [p for p in range(len(pairs)) if base[p] != want[p]]
    assert not bad, (len(bad), bad[:5], base[bad[0]], want[bad[0]])
    return batch, sc, want


def cigar_of_strings(ra: bytes, rb: bytes, extended: int, fold: int) -> bytes:
    lib = S.lib()
    lib.seqalign_cigar.restype = C.c_size_t
    out = C.create_string_buffer(2 * len(ra) + 8)
    n = lib.seqalign_cigar(ra, rb, C.c_size_t(len(ra)), C.c_int(extended), C.c_int(fold), out, C.c_size_t(len(out)))
    assert n != C.c_size_t(-1).value
    return out.value


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(NW_ROUTES))
def test_nw_batch_pipeline_shapes_small_ragged(ctx, opts, small_ragged, route):
    """Every way through the chunk pipeline that a small batch can be made to take: the result forms (moves home staged or in
    place, strings home, three matrices) crossed with 1 / 2 / 5 sub-batches, walk_overlap on or off (one group here: the walks
    run beside fills in test_nw_batch_more_than_one_group), 1 / 4 upload
    slices asked for (one runs at this size; more: test_nw_batch_upload_slices), packed fills forced or off -- on 1 300 pairs of lengths 0 .. 40 (empty sequences, runs of one tiny shape) in more than
    two host blocks, half of them `packed` in the caller's arena and half not.  Every result equals the default route's, which
    equals the oracle's for every pair; the CIGAR call (both formats) equals seqalign_cigar of the oracle's strings."""
    batch, sc, want = small_ragged
    for n_sub, overlap, slices, pk in NW_PIPELINE_SHAPES:
        opts(subbatches=n_sub, walk_overlap=overlap, upload_slices=slices, pack16=pk, **NW_ROUTES[route])
        got = ctx.nw_batch(batch, sc)
        ran = ctx.last_call()
        assert any(k.startswith("fill_nw_dirs") for k in ran) == (route != "nw_dirs=0"), (route, ran)
        assert any(k.startswith("walk_moves_") for k in ran) == (route not in ("nw_dirs=0", "nw_moves=0")), (route, ran)
        bad = [p for p in range(batch.n_pairs) if got[p] != want[p]]
        assert not bad, (route, n_sub, overlap, slices, pk, len(bad), bad[:5], got[bad[0]], want[bad[0]])
    if route in ("default", "nw_dirs=0"):
        fold = int(not sc.case_sensitive)
        for fmt in (1, 2):   # SEQALIGN_CIGAR_M, SEQALIGN_CIGAR_EQX
            for n_sub, overlap, slices, pk in ((0, 0, 1, 0), (5, 1, 4, 2)):
                opts(subbatches=n_sub, walk_overlap=overlap, upload_slices=slices, pack16=pk)
                got = ctx.nw_batch_cigar(batch, sc, fmt=fmt)
                bad = [p for p in range(batch.n_pairs) if got[p] != (want[p][0], cigar_of_strings(want[p][1], want[p][2], int(fmt == 2), fold))]
                assert not bad, (route, fmt, n_sub, len(bad), bad[:5], got[bad[0]], want[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["default", "zero_copy=0", "zero_copy=2"])
def test_nw_batch_upload_slices(ctx, opts, route):
    """The moves form's sliced upload (option upload_slices: a sub-batch's sequences are packed and sent slice by slice, at most one
    slice per two host blocks): 4 200 pairs of lengths 0 .. 40 are 9 host blocks of 512 in one sub-batch (2 and 4 slices) and 17 blocks
    of 256 in two (4 slices each), the first half of the pairs `packed` in the caller's arena, the second half not, one block both.
    Every result equals the oracle's and the unsliced call's."""
    batch, pairs = NB.half_packed_ragged(n=4200, seed=4242)
    sc = S.make_scoring({"preset": "default"})
    osc = oracle_scoring_of(sc)
    want = []
    for a, b in pairs:
        rc, s_, ra, rb = O.oracle_nw(osc, a, b)
        assert rc == 0
        want.append((s_, ra, rb))
    opts(**NW_ROUTES[route])
    assert ctx.nw_batch(batch, sc) == want
    for n_sub, slices in ((0, 2), (0, 4), (0, 16), (2, 4)):
        opts(subbatches=n_sub, upload_slices=slices)
        got = ctx.nw_batch(batch, sc)
        bad = [p for p in range(batch.n_pairs) if got[p] != want[p]]
        assert not bad, (route, n_sub, slices, len(bad), bad[:5], got[bad[0]], want[bad[0]])


def nw_raw_copy(ctx, batch, sc):
    str_off, out_a, out_b, out_len, out_score = ctx.nw_batch(batch, sc, raw=True)
    return str_off, out_a.copy(), out_b.copy(), out_len.copy(), out_score.copy()


def nw_raw_pair(raw, p):
    str_off, out_a, out_b, out_len, out_score = raw
    o, ln = int(str_off[p]), int(out_len[p])
    return int(out_score[p]), out_a[o:o + ln].tobytes(), out_b[o:o + ln].tobytes()


# what a call launches on 65 536 pairs in four sub-batches: {kernel kind: (launches, pairs)} per (batch, nw_moves), the same with
# the walks beside the fills and behind them (read off the library before the two pipelines became one driver: 4 fills, 2 walks).
# The ragged batch's mixed grids count under both kinds, one launch each per sub-batch; with strings home it has no majority shape
# and nothing is packed.
NW_GROUP_LAUNCHES = {
    ("one_shape", 1): {"fill_nw_dirs_x4": (4, 65536), "walk_moves_tile": (2, 65536)},
    ("one_shape", 0): {"fill_nw_dirs_x4": (4, 65536), "walk_dirs_lane": (2, 65536)},
    ("ragged", 1): {"fill_nw_dirs": (4, 350), "fill_nw_dirs_x2": (4, 65186), "walk_moves_tile": (2, 65536)},
    ("ragged", 0): {"fill_nw_dirs": (4, 65536), "walk_dirs_lane": (2, 65536)},
}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["one_shape", "ragged"])
def test_nw_batch_more_than_one_group(ctx, opts, kind):
    """A pipeline of more than one GROUP (>= 32 768 pairs per group: sa_batch.hip): 65 536 pairs of 12 x 10 in four sub-batches of
    whole rounds (cuts at 16 384, 32 768, 49 152: two groups), and a ragged twin of lengths 4 .. 16 cut at equal cells; moves home
    and strings home, the first group's walk beside the second group's fills and behind them.  The four settings agree, every
    257th pair equals the oracle's, and the fills' and walks' launch and pair counts are the recorded ones."""
    n = 65536
    if kind == "one_shape":
        rng = W.Rng(31)
        a = W.DNA[rng.below(4, n * 12).astype(np.int64)].reshape(n, 12)
        b = W.DNA[rng.below(4, n * 10).astype(np.int64)].reshape(n, 10)
        b[:, :8] = np.where(rng.unit(n * 8).reshape(n, 8) < 0.8, a[:, 2:10], b[:, :8])
        batch = W._fixed_batch(a, b)
    else:
        batch = NB.ragged_related(n, 4, 16, seed=32)
    sc = S.make_scoring({"preset": "default"})
    osc = oracle_scoring_of(sc)
    first, launched = None, {}
    for moves, overlap in ((1, 1), (1, 0), (0, 1), (0, 0)):
        opts(subbatches=4, nw_moves=moves, walk_overlap=overlap)
        raw = nw_raw_copy(ctx, batch, sc)
        ran = ctx.last_call()
        print(f"launches {kind} nw_moves={moves} walk_overlap={overlap}: {ran}")
        if first is None:
            first = raw
            for p in range(0, n, 257):
                rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
                assert rc == 0 and nw_raw_pair(raw, p) == (s_, ra, rb), (kind, p)
        else:
            assert all(np.array_equal(x, y) for x, y in zip(raw[3:], first[3:])), (kind, moves, overlap)
            ends = raw[0] + raw[3].astype(np.uint64)
            for x, y in zip(raw[1:3], first[1:3]):   # (bytes behind a string's NUL are unspecified: compare the strings)
                diff = np.nonzero(x != y)[0]
                if diff.size:
                    owner = np.searchsorted(raw[0], diff, side="right") - 1
                    assert np.all(diff.astype(np.uint64) > ends[owner]), (kind, moves, overlap, int(diff[0]))
        launched[moves, overlap] = ran
    for (moves, overlap), ran in launched.items():
        fills = {k: v for k, v in ran.items() if k.startswith("fill_")}
        assert all(v[0] == 4 for v in fills.values()) and sum(v[1] for v in fills.values()) == n, (kind, moves, overlap, ran)
        assert ran == NW_GROUP_LAUNCHES[kind, moves], (kind, moves, overlap, ran)


def mostly_one_shape_pairs(rng, n):
    def rand(m):
        return bytes(b"ACGT"[i] for i in rng.below(4, m)) if m else b""
    pairs = []
    for k in range(n):
        la, lb = (int(rng.below(160, 1)[0]), int(rng.below(160, 1)[0])) if k % 7 == 3 else (100, 100)
        a = rand(la)
        pairs.append((a, (a[:lb] + rand(max(0, lb - la))) if k % 2 else rand(lb)))
    return pairs


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mostly_one_shape", "mostly_one_shape_forced", "every_length", "table_too_large"])
def test_nw_batch_strings_form_on_ragged_packable_chunks(ctx, opts, case):
    """nw_moves = 0 (strings come home) on ragged chunks the packed fill may take: which pairs go two per wave is the chunk
    layout's choice (this form's: the majority shape's pairs, sa_batch.hip: majority_vote_layout) and never shows in the results --
    equal to pack16 = 0 and to the oracle on every 23rd pair.  mostly one shape: test_nw_batch_mostly_one_shape's batch, 2 600 pairs at pack16 = 1 and 90 forced;
    every length 100 .. 150: no majority shape; table too large: a majority of 100 x 100 that the packed fill takes beside one
    pair of 1 023 x 10 and one of 10 x 1 100, whose (max_a + 1) (max_b + 1) is beyond the moves form's pairing table.  (No launch counts:
    the mix of waves is the layout rule's business.)"""
    rng = W.Rng(777)
    n, pk = 2600, 1
    if case == "mostly_one_shape":
        batch = W.from_pairs(mostly_one_shape_pairs(rng, n))
    elif case == "mostly_one_shape_forced":
        n, pk = 90, 2
        batch = W.from_pairs(mostly_one_shape_pairs(rng, n))
    elif case == "every_length":
        batch = NB.ragged_related(n, 100, 150, seed=778)
    else:
        pairs = mostly_one_shape_pairs(rng, n)
        pairs[23] = (pairs[23][0] * 11)[:1023], pairs[23][1][:10]
        pairs[46] = pairs[46][0][:10], (pairs[46][1] * 12)[:1100]
        assert len(pairs[23][0]) == 1023 and len(pairs[46][1]) == 1100
        batch = W.from_pairs(pairs)
    sc = S.make_scoring({"preset": "default"})
    osc = oracle_scoring_of(sc)
    for n_sub in (0, 3):
        opts(nw_moves=0, pack16=pk, subbatches=n_sub)
        got = ctx.nw_batch(batch, sc)
        ran = ctx.last_call()
        assert any(k.startswith("fill_nw_dirs") for k in ran) and not any(k.startswith("walk_moves_") for k in ran), ran
        opts(nw_moves=0, pack16=0, subbatches=n_sub)
        assert got == ctx.nw_batch(batch, sc), (case, n_sub)
        for p in range(0, n, 1 if n < 200 else 23):
            rc, s_, ra, rb = O.oracle_nw(osc, batch.seq_a(p), batch.seq_b(p))
            assert rc == 0 and got[p] == (s_, ra, rb), (case, n_sub, p)
