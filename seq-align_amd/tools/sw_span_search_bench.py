#!/usr/bin/env python3
"""sw_span_search_bench.py -- the SW hit-span calls over two sets (seqalign_sw_span_cross, seqalign_sw_span_search) next to what
they replace and what they are built from, on the same sets, one workload per process.

Workloads:
  c4   64 protein queries x 4 000 targets of about 300 aa, BLOSUM62
  c3   1 000 reads of 150 bp x 1 000 windows of 1 000 bp, match 2 / mismatch -2 / gap -2 -1

One JSON line.  Every *_ms entry is {"median", "min", "max"} of --calls whole calls (wall clock: host arrays in, host arrays out):
  span_cross_ms        seqalign_sw_span_cross
  span_batch_ms        seqalign_sw_span_batch on the explicit Q x T batch of the same pairs (batch_build_ms: building that batch
                       on the host, once, not part of the call)
  score_cross_ms       seqalign_sw_score_cross; span_over_score_cross: the ratio of the two cross calls' medians
  span_search_ms       seqalign_sw_span_search, k = --k
  score_search_ms      seqalign_sw_score_search on the same arguments
  span_hits_ms         seqalign_sw_span_batch on the batch of the selected hit pairs UNTRUNCATED (whole query, whole target)
  span_prefix_ms       seqalign_sw_span_batch on the same pairs cut at their best cells, the list stage 2 builds (prefix_launches:
                       how many launches that list takes, untruncated_launches: the untruncated one)
  stage2_share         (span_search - score_search) / span_search, from the medians
Aims, set before anything ran and recorded as met or missed (no margin beyond the recorded spread):
  aim_cross_met        span_cross <= span_batch
  aim_search_met       span_search <= score_search + span_hits
Before the line is printed the tool ASSERTS that the span matrices equal the explicit batch's result, that the search's
targets and scores are the score search's and that its spans are the matrices' entries; it exits non-zero otherwise.

    python seq-align_amd/tools/sw_span_search_bench.py --workload c4 [--calls 10] [--k 10] [--scale 1]
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


def sets_of(name, scale):
    if name == "c4":
        spec = {"preset": "BLOSUM62"}
        q = W.random_set(max(1, 64 // scale), 401, 270, 330, bytes(W.AMINO20))
        t = W.random_set(max(1, 4000 // scale), 402, 270, 330, bytes(W.AMINO20))
    elif name == "c3":
        spec = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}
        q = W.random_set(max(1, 1000 // scale), 301, 150, 150)
        t = W.random_set(max(1, 1000 // scale), 302, 1000, 1000)
    else:
        raise SystemExit(f"unknown workload {name}")
    return spec, q, t


def timed(fn, calls, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=["c4", "c3"])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the set sizes (a quick run)")
    args = ap.parse_args()
    spec, q, t = sets_of(args.workload, args.scale)
    sc = S.make_scoring(spec)
    nq, nt, k = q.n_seqs, t.n_seqs, args.k
    cells = int(q.len.astype(np.int64).sum()) * int(t.len.astype(np.int64).sum())
    with S.Context(0) as ctx:
        # results first
        t0 = time.perf_counter()
        batch = W.cross_batch(q, t)
        build_ms = (time.perf_counter() - t0) * 1e3
        dense = ctx.sw_span_cross(q, t, sc)
        cross_launches = ctx.last_call()
        want = ctx.sw_span(batch, sc)
        assert all(np.array_equal(g.reshape(-1), w) for g, w in zip(dense, want)), "the span matrices differ from the explicit batch's result"
        n_hits, hits = ctx.sw_span_search(q, t, sc, k)
        search_launches = ctx.last_call()
        n_score, score_hits = ctx.sw_score_search(q, t, sc, k)
        assert np.array_equal(n_hits, n_score), "n_hits differ from the score search's"
        pick = [(i, int(h["target"])) for i in range(nq) for h in hits[i, :int(n_hits[i])]]
        for i in range(nq):
            h, s = hits[i, :int(n_hits[i])], score_hits[i, :int(n_hits[i])]
            assert np.array_equal(h["target"], s["target"]) and np.array_equal(h["score"], s["score"]), ("query", i)
            for name, m in zip(("score", "pos_a", "pos_b", "len_a", "len_b"), dense):
                assert np.array_equal(h[name], m[i][h["target"]]), ("query", i, name)
        hit_batch = W.from_pairs([(q.seq(i), t.seq(j)) for i, j in pick])
        ends = [(int(h["pos_a"] + h["len_a"]), int(h["pos_b"] + h["len_b"])) for i in range(nq) for h in hits[i, :int(n_hits[i])]]
        prefix_batch = W.from_pairs([(q.seq(i)[:ea], t.seq(j)[:eb]) for (i, j), (ea, eb) in zip(pick, ends)])
        ctx.sw_span(hit_batch, sc)
        untruncated_launches = sum(v[0] for v in ctx.last_call().values())
        ctx.sw_span(prefix_batch, sc)
        prefix_launches = sum(v[0] for v in ctx.last_call().values())

        out = {"workload": args.workload, "queries": nq, "targets": nt, "k": k, "cells": cells, "timed_calls": args.calls,
               "hits": len(pick), "batch_build_ms": round(build_ms, 3)}
        out["span_cross_ms"] = timed(lambda: ctx.sw_span_cross(q, t, sc), args.calls)
        out["span_batch_ms"] = timed(lambda: ctx.sw_span(batch, sc), args.calls)
        out["score_cross_ms"] = timed(lambda: ctx.sw_score_cross(q, t, sc), args.calls)
        out["span_search_ms"] = timed(lambda: ctx.sw_span_search(q, t, sc, k), args.calls)
        out["score_search_ms"] = timed(lambda: ctx.sw_score_search(q, t, sc, k), args.calls)
        out["span_hits_ms"] = timed(lambda: ctx.sw_span(hit_batch, sc), args.calls)
        out["span_prefix_ms"] = timed(lambda: ctx.sw_span(prefix_batch, sc), args.calls)
        out["untruncated_launches"], out["prefix_launches"] = untruncated_launches, prefix_launches
        out["prefix_cells_share"] = round(prefix_batch.cells() / max(1, hit_batch.cells()), 4)
    med = lambda key: out[key]["median"]
    out["span_cross_gcups"] = round(cells / (med("span_cross_ms") * 1e-3) / 1e9, 1)
    out["span_over_score_cross"] = round(med("span_cross_ms") / med("score_cross_ms"), 3)
    out["stage2_share"] = round((med("span_search_ms") - med("score_search_ms")) / med("span_search_ms"), 4)
    out["equals_explicit_batch"] = out["equals_score_search"] = True
    out["launches"] = {"span_cross": {n: v[0] for n, v in cross_launches.items()}, "span_search": {n: v[0] for n, v in search_launches.items()}}
    out["aim_cross_met"] = bool(med("span_cross_ms") <= med("span_batch_ms"))
    out["aim_search_met"] = bool(med("span_search_ms") <= med("score_search_ms") + med("span_hits_ms"))
    print(json.dumps(out), flush=True)
    for aim, what in (("aim_cross_met", "span cross is slower than sw_span on the explicit batch"),
                      ("aim_search_met", "span search takes longer than the score search plus sw_span on the untruncated hit pairs")):
        if not out[aim]:
            print(f"workload {args.workload}: AIM MISSED: {what}", file=sys.stderr, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
