#!/usr/bin/env python3
"""nw_stats_bench.py -- the NW statistics calls (seqalign_nw_stats_batch, seqalign_nw_stats_cross) next to what they replace and
what they are built from, on the same batch, one workload per process.

Workloads:
  c2      10 000 pairs of 150 x 150 DNA, match 1 / mismatch -2 / gap -4 -1
  b62     4 000 pairs of 300 x 300 aa, BLOSUM62
  long    64 pairs of 5 000 x 5 000 DNA (the strips)
  one     one pair of 60 000 x 60 000 DNA (past the alignment calls' 2^31-cell cap)
  cross   64 protein queries x 4 000 targets of about 300 aa, BLOSUM62: the cross call

One JSON line.  *_kernel_ms: {"median", "min", "max"} of --launches launches between HIP events (seqalign_nw_stats_time_ms,
seqalign_score_time_ms, seqalign_sw_span_time_ms; the batch uploaded once).  *_call_ms: the same of --calls whole calls (wall clock:
host arrays in, host arrays out):
  stats_*            seqalign_nw_stats_batch
  nw_score_*         seqalign_nw_score_batch
  sw_span_*          seqalign_sw_span_batch under the same scoring
  align_count_call_ms   seqalign_nw_batch (one: seqalign_nw_align_long) plus counting the columns of its strings on the host
  cross: stats_cross_call_ms, stats_batch_call_ms (seqalign_nw_stats_batch on the explicit Q x T batch; batch_build_ms: building
         it, once, not part of the call), score_cross_call_ms (seqalign_nw_score_cross)
Aims, set before anything ran and recorded as met or missed (no margin beyond the recorded spread):
  aim_kernel_met     stats_kernel_ms <= sw_span_kernel_ms (medians)
  aim_cross_met      stats_cross_call_ms <= stats_batch_call_ms (medians)
Before the line is printed the tool ASSERTS that the scores equal seqalign_nw_score_batch's, that the counts equal those of the
alignment call's strings (c2, b62, long: a sample of 64 pairs; one: the pair), and that the matrices equal the explicit batch's
result; it exits non-zero otherwise.

    python seq-align_amd/tools/nw_stats_bench.py --workload c2 [--launches 20] [--calls 10] [--scale 1]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python")]

import seqalign_amd as S                                   # noqa: E402
from seqalign_amd import workloads as W                    # noqa: E402

DNA = {"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]}


def related_dna(n_pairs, length, seed):
    """Pairs of `length`: seq_b is seq_a with about 4 % substitutions and a few short indels."""
    rng = W.Rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for _ in range(n_pairs):
        a = letters[rng.below(4, length).astype(np.int64)].copy()
        b = a.copy()
        at = rng.below(length, length // 25).astype(np.int64)
        b[at] = letters[rng.below(4, len(at)).astype(np.int64)]
        cut = np.sort(rng.below(length, 8).astype(np.int64))
        b = np.delete(b, np.concatenate([np.arange(c, min(length, c + 5)) for c in cut[:4]]))
        b = np.insert(b, np.minimum(cut[4:], len(b)), letters[rng.below(4, 4).astype(np.int64)])
        pairs.append((a.tobytes(), b.tobytes()))
    return W.from_pairs(pairs)


def batch_of(name, scale):
    if name == "c2":
        return DNA, W.dna_nw_150(max(1, 10000 // scale), seed=1)
    if name == "b62":
        return {"preset": "BLOSUM62"}, W.protein_sw_300(max(1, 4000 // scale), seed=3)
    if name == "long":
        return DNA, related_dna(max(1, 64 // scale), 5000 // scale, 64)
    if name == "one":
        return DNA, related_dna(1, 60000 // scale, 60)
    raise SystemExit(f"unknown workload {name}")


def spread(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(min(ts)), 4), "max": round(float(max(ts)), 4)}


def timed(fn, calls, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def fold(sc, s):
    return s if sc.case_sensitive else s.lower()


def count_columns(sc, ra, rb):
    fa, fb = np.frombuffer(fold(sc, ra), np.uint8), np.frombuffer(fold(sc, rb), np.uint8)
    both = (np.frombuffer(ra, np.uint8) != 45) & (np.frombuffer(rb, np.uint8) != 45)
    m = int(np.count_nonzero(both & (fa == fb)))
    return m, int(np.count_nonzero(both)) - m


def run_batch(ctx, name, args):
    spec, batch = batch_of(name, args.scale)
    sc = S.make_scoring(spec)
    cells = int((batch.len_a.astype(np.int64) * batch.len_b.astype(np.int64)).sum())
    out = {"workload": name, "pairs": batch.n_pairs, "cells": cells, "launches": args.launches, "calls": args.calls}
    align = ctx.nw_align_long if name == "one" else ctx.nw_batch

    def align_and_count():
        return [(s,) + count_columns(sc, ra, rb) for s, ra, rb in align(batch, sc)]

    score, m, mm = ctx.nw_stats(batch, sc)
    out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
    assert np.array_equal(score, ctx.nw_score(batch, sc)), "scores differ from nw_score"
    sample = batch if batch.n_pairs <= 64 else W.from_pairs([(batch.seq_a(p), batch.seq_b(p)) for p in range(0, batch.n_pairs, batch.n_pairs // 64)][:64])
    step = 1 if batch.n_pairs <= 64 else batch.n_pairs // 64
    for k, (s, ra, rb) in enumerate(align(sample, sc)):
        p = k * step
        assert (int(score[p]), int(m[p]), int(mm[p])) == (s,) + count_columns(sc, ra, rb), f"pair {p}: counts differ from the strings'"
    out["identity_mean"] = round(float(np.mean(m / np.maximum(1, batch.len_a.astype(np.int64) + batch.len_b - m - mm))), 4)

    out["stats_kernel_ms"] = spread(ctx.nw_stats_time_ms(batch, sc, repeats=args.launches))
    out["nw_score_kernel_ms"] = spread(ctx.score_time_ms(batch, sc, 0, repeats=args.launches))
    out["sw_span_kernel_ms"] = spread(ctx.sw_span_time_ms(batch, sc, repeats=args.launches))
    out["stats_gcups"] = round(cells / out["stats_kernel_ms"]["median"] / 1e6, 1)
    out["stats_call_ms"] = timed(lambda: ctx.nw_stats(batch, sc), args.calls)
    out["nw_score_call_ms"] = timed(lambda: ctx.nw_score(batch, sc), args.calls)
    out["sw_span_call_ms"] = timed(lambda: ctx.sw_span(batch, sc), args.calls)
    out["align_count_call_ms"] = timed(align_and_count, max(2, args.calls // 3 if name in ("long", "one") else args.calls))
    out["stats_over_span_kernel"] = round(out["stats_kernel_ms"]["median"] / out["sw_span_kernel_ms"]["median"], 3)
    out["stats_over_score_kernel"] = round(out["stats_kernel_ms"]["median"] / out["nw_score_kernel_ms"]["median"], 3)
    out["align_count_over_stats_call"] = round(out["align_count_call_ms"]["median"] / out["stats_call_ms"]["median"], 2)
    out["aim_kernel_met"] = out["stats_kernel_ms"]["median"] <= out["sw_span_kernel_ms"]["median"]
    return out


def run_cross(ctx, args):
    sc = S.make_scoring({"preset": "BLOSUM62"})
    q = W.random_set(max(1, 64 // args.scale), 401, 270, 330, bytes(W.AMINO20))
    t = W.random_set(max(1, 4000 // args.scale), 402, 270, 330, bytes(W.AMINO20))
    cells = int(q.len.astype(np.int64).sum()) * int(t.len.astype(np.int64).sum())
    out = {"workload": "cross", "queries": q.n_seqs, "targets": t.n_seqs, "cells": cells, "calls": args.calls}
    t0 = time.perf_counter()
    explicit = W.cross_batch(q, t)
    out["batch_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    got = ctx.nw_stats_cross(q, t, sc)
    out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
    want = ctx.nw_stats(explicit, sc)
    assert all(np.array_equal(g.ravel(), w) for g, w in zip(got, want)), "matrices differ from the explicit batch's result"
    assert np.array_equal(got[0], ctx.nw_score_cross(q, t, sc)), "scores differ from nw_score_cross"
    out["stats_cross_call_ms"] = timed(lambda: ctx.nw_stats_cross(q, t, sc), args.calls)
    out["stats_batch_call_ms"] = timed(lambda: ctx.nw_stats(explicit, sc), args.calls)
    out["score_cross_call_ms"] = timed(lambda: ctx.nw_score_cross(q, t, sc), args.calls)
    out["stats_batch_kernel_ms"] = spread(ctx.nw_stats_time_ms(explicit, sc, repeats=args.launches))
    out["cross_gcups_call"] = round(cells / out["stats_cross_call_ms"]["median"] / 1e6, 1)
    out["stats_over_score_cross"] = round(out["stats_cross_call_ms"]["median"] / out["score_cross_call_ms"]["median"], 3)
    out["aim_cross_met"] = out["stats_cross_call_ms"]["median"] <= out["stats_batch_call_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=["c2", "b62", "long", "one", "cross"])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the sizes (a quick run)")
    args = ap.parse_args()
    with S.Context(0) as ctx:
        out = run_cross(ctx, args) if args.workload == "cross" else run_batch(ctx, args.workload, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
