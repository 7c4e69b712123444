#!/usr/bin/env python3
"""sw_stats_bench.py -- the SW statistics calls (seqalign_sw_stats_batch, seqalign_sw_stats_cross) next to what they replace and
what they are built from, on the same batch, one workload per process.

Workloads:
  c3      10 000 reads of 150 bp in 400 bp windows, match 2 / mismatch -2 / gap -2 -1
  c4      4 000 pairs of 300 x 300 aa, BLOSUM62
  reads   10 000 reads of 700 bp in 1 000 bp windows (the strips: two per pair)
  long    64 related pairs of 5 000 x 5 000 DNA
  one     one related pair of 60 000 x 60 000 DNA (past the alignment calls' 2^31-cell cap, inside the 65 535-letter limit)
  cross   64 protein queries x 4 000 targets of about 300 aa, BLOSUM62: the cross call

One JSON line.  *_kernel_ms: {"median", "min", "max"} of --launches launches between HIP events (seqalign_sw_stats_time_ms,
seqalign_sw_span_time_ms, seqalign_score_time_ms; the batch uploaded once).  *_call_ms: the same of --calls whole calls (wall clock:
host arrays in, host arrays out):
  stats_*            seqalign_sw_stats_batch
  sw_span_*          seqalign_sw_span_batch
  sw_score_*         seqalign_sw_score_batch
  align_count_call_ms   seqalign_sw_batch(min_score = 1, max_hits = 1) (one: seqalign_sw_align_long) plus counting the columns of
                     its strings on the host
  cross: stats_cross_call_ms, stats_batch_call_ms (seqalign_sw_stats_batch on the explicit Q x T batch; batch_build_ms: building
         it, once, not part of the call), span_cross_call_ms (seqalign_sw_span_cross)
Aims, set before anything ran and recorded as met or missed; a result inside the spread of the two medians is `level`:
  aim_kernel         stats_kernel_ms <= sw_span_kernel_ms (medians)
  aim_call_met       stats_call_ms < align_count_call_ms (medians)
  aim_cross_met      stats_cross_call_ms <= stats_batch_call_ms (medians)
Before the line is printed the tool ASSERTS that the first five outputs are seqalign_sw_span_batch's bit for bit, that the counts
equal those of the alignment call's strings (a sample of 64 pairs; long: 8; one: the pair), and that the matrices equal the
explicit batch's result; it exits non-zero otherwise.

    python seq-align_amd/tools/sw_stats_bench.py --workload c3 [--launches 20] [--calls 10] [--scale 1]
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

DNA_SW = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}
WORKLOADS = ["c3", "c4", "reads", "long", "one", "cross"]


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
    if name == "c3":
        return DNA_SW, W.dna_sw_read_vs_ref(max(1, 10000 // scale), seed=2)
    if name == "c4":
        return {"preset": "BLOSUM62"}, W.protein_sw_300(max(1, 4000 // scale), seed=3)
    if name == "reads":
        return DNA_SW, W.dna_sw_read_vs_ref(max(1, 10000 // scale), seed=4, read_len=700, ref_len=1000)
    if name == "long":
        return DNA_SW, related_dna(max(1, 64 // scale), 5000 // scale, 64)
    if name == "one":
        return DNA_SW, related_dna(1, 60000 // scale, 60)
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


def verdict(ours, theirs, strict=False):
    """met / missed by the medians; `level` where each median lies inside the other's spread."""
    if ours["min"] <= theirs["median"] <= ours["max"] and theirs["min"] <= ours["median"] <= theirs["max"]:
        return "level"
    ok = ours["median"] < theirs["median"] if strict else ours["median"] <= theirs["median"]
    return "met" if ok else "missed"


def fold(sc, s):
    return s if sc.case_sensitive else s.lower()


def count_columns(sc, ra, rb):
    fa, fb = np.frombuffer(fold(sc, ra), np.uint8), np.frombuffer(fold(sc, rb), np.uint8)
    both = (np.frombuffer(ra, np.uint8) != 45) & (np.frombuffer(rb, np.uint8) != 45)
    m = int(np.count_nonzero(both & (fa == fb)))
    return m, int(np.count_nonzero(both)) - m


def hit_fields(sc, hits):
    if not hits:
        return (0,) * 7
    h = hits[0]
    return (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) + count_columns(sc, h["a"].encode(), h["b"].encode())


def run_batch(ctx, name, args):
    spec, batch = batch_of(name, args.scale)
    sc = S.make_scoring(spec)
    cells = int((batch.len_a.astype(np.int64) * batch.len_b.astype(np.int64)).sum())
    out = {"workload": name, "pairs": batch.n_pairs, "cells": cells, "launches": args.launches, "calls": args.calls}
    too_large = bool(((batch.len_a.astype(np.int64) + 1) * (batch.len_b.astype(np.int64) + 1) >= 2 ** 31).any())
    out["align_call"] = "sw_align_long" if too_large else "sw_batch(max_hits=1)"

    def align(b):
        return ctx.sw_align_long(b, sc, 1) if too_large else ctx.sw_batch(b, sc, 1, max_hits=1)

    def align_and_count():
        return [hit_fields(sc, h) for h in align(batch)]

    got = ctx.sw_stats(batch, sc)
    out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:5], ctx.sw_span(batch, sc))), "the first five outputs differ from sw_span's"
    n_sample = 8 if name == "long" else 64
    step = max(1, batch.n_pairs // n_sample)
    picks = list(range(0, batch.n_pairs, step))[:n_sample]
    sample = W.from_pairs([(batch.seq_a(p), batch.seq_b(p)) for p in picks])
    for p, h in zip(picks, align(sample)):
        assert tuple(int(x[p]) for x in got) == hit_fields(sc, h), f"pair {p}: differs from the alignment call's hit"
    m, mm = got[5].astype(np.int64), got[6].astype(np.int64)
    length = got[3].astype(np.int64) + got[4] - m - mm
    out["identity_mean"] = round(float(np.mean(m / np.maximum(1, length))), 4)

    out["stats_kernel_ms"] = spread(ctx.sw_stats_time_ms(batch, sc, repeats=args.launches))
    out["sw_span_kernel_ms"] = spread(ctx.sw_span_time_ms(batch, sc, repeats=args.launches))
    out["sw_score_kernel_ms"] = spread(ctx.score_time_ms(batch, sc, 1, repeats=args.launches))
    out["stats_gcups"] = round(cells / out["stats_kernel_ms"]["median"] / 1e6, 1)
    out["stats_call_ms"] = timed(lambda: ctx.sw_stats(batch, sc), args.calls)
    out["sw_span_call_ms"] = timed(lambda: ctx.sw_span(batch, sc), args.calls)
    out["sw_score_call_ms"] = timed(lambda: ctx.sw_score(batch, sc), args.calls)
    out["align_count_call_ms"] = timed(align_and_count, max(2, args.calls // 3 if name in ("long", "one") else args.calls))
    out["stats_over_span_kernel"] = round(out["stats_kernel_ms"]["median"] / out["sw_span_kernel_ms"]["median"], 3)
    out["stats_over_score_kernel"] = round(out["stats_kernel_ms"]["median"] / out["sw_score_kernel_ms"]["median"], 3)
    out["align_count_over_stats_call"] = round(out["align_count_call_ms"]["median"] / out["stats_call_ms"]["median"], 2)
    out["aim_kernel"] = verdict(out["stats_kernel_ms"], out["sw_span_kernel_ms"])
    out["aim_call_met"] = out["stats_call_ms"]["median"] < out["align_count_call_ms"]["median"]
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
    got = ctx.sw_stats_cross(q, t, sc)
    out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
    want = ctx.sw_stats(explicit, sc)
    assert all(np.array_equal(g.ravel(), w) for g, w in zip(got, want)), "matrices differ from the explicit batch's result"
    assert all(np.array_equal(g, w) for g, w in zip(got[:5], ctx.sw_span_cross(q, t, sc))), "the first five differ from sw_span_cross"
    out["stats_cross_call_ms"] = timed(lambda: ctx.sw_stats_cross(q, t, sc), args.calls)
    out["stats_batch_call_ms"] = timed(lambda: ctx.sw_stats(explicit, sc), args.calls)
    out["span_cross_call_ms"] = timed(lambda: ctx.sw_span_cross(q, t, sc), args.calls)
    out["stats_batch_kernel_ms"] = spread(ctx.sw_stats_time_ms(explicit, sc, repeats=args.launches))
    out["cross_gcups_call"] = round(cells / out["stats_cross_call_ms"]["median"] / 1e6, 1)
    out["stats_over_span_cross"] = round(out["stats_cross_call_ms"]["median"] / out["span_cross_call_ms"]["median"], 3)
    out["aim_cross_met"] = out["stats_cross_call_ms"]["median"] <= out["stats_batch_call_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=WORKLOADS)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the sizes (a quick run)")
    args = ap.parse_args()
    with S.Context(0) as ctx:
        out = run_cross(ctx, args) if args.workload == "cross" else run_batch(ctx, args.workload, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
