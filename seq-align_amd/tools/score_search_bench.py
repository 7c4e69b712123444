#!/usr/bin/env python3
"""score_search_bench.py -- the top-k score search (seqalign_nw_score_search / seqalign_sw_score_search), and on the same sets
the score-matrix call followed by a host top-k (np.lexsort per row), in one process.

Workloads (seeded):
  S1   all-vs-all SW, BLOSUM62: 2 000 proteins of length 100-500 against themselves, k = 10, min_score 1 (score_cross_bench's X1)
  S2   SW, BLOSUM62: 64 protein queries against 500 000 targets of 100-500, k = 20, min_score 1
  S3   NW, default DNA scoring: 1 000 reads of 150 against 100 000 reads of 150, k = 5, no cut

One JSON line per workload:
  call_ms        median wall clock of the synchronous search call (host sets in, hit lists out), after `--warm` calls
  gcups          len_a x len_b cells / call_ms
  h2d_bytes      sequences and descriptors sent (each set's bytes once per tile, 16 B per sequence; one tile assumed)
  d2h_bytes      what comes home: n_queries x (k x 16 + 4) B of lists and counts (plus 16 B per tile of error words)
  cross_d2h_bytes  what the matrix call brings home instead: 4 (NW) / 12 (SW) B per pair
  launches       what the search launched (seqalign_ctx_last_call_info)
  cross_call_ms, host_topk_ms  the matrix call, and the host top-k over its result (unless --no-cross; S2's matrices are
                 384 MB, S3's 400 MB)
  identical      the search's hits equal the host top-k's
Kernel times: a run of its own under `rocprofv3 --kernel-trace --stats` (score_rows_kernel<..., true> is the sweep,
score_select_kernel the selection); per call = total / (calls + warm).

    python seq-align_amd/tools/score_search_bench.py [--only S1,S2] [--calls 3] [--warm 1] [--no-cross]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python"), str(ROOT / "tests")]

import seqalign_amd as S                      # noqa: E402
from seqalign_amd import workloads as W       # noqa: E402

PROTEIN, DNA = bytes(W.AMINO20), b"ACGT"


def workloads():
    blosum, dna = {"preset": "BLOSUM62"}, {"preset": "default"}

    def s1():
        p = W.random_set(2000, 1, 100, 500, PROTEIN)
        return p, p
    yield "S1", s1, blosum, 1, 10, 1
    yield "S2", lambda: (W.random_set(64, 11, 100, 500, PROTEIN), W.random_set(500_000, 12, 100, 500, PROTEIN)), blosum, 1, 20, 1
    yield "S3", lambda: (W.random_set(1000, 13, 150, 150, DNA), W.random_set(100_000, 14, 150, 150, DNA)), dna, 0, 5, S.INT32_MIN


def cells(q, t):
    return int(q.len.astype(np.int64).sum()) * int(t.len.astype(np.int64).sum())


def median_ms(fn, calls, warm):
    for _ in range(warm):
        fn()
    ts, out = [], None
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def host_top_k(score, end_a, end_b, k, min_score):
    """Per row: the contract by np.lexsort, as (n_hits, hits) of the search call."""
    nq = score.shape[0]
    n_hits, hits = np.zeros(nq, np.uint32), np.zeros((nq, k), S.SEARCH_HIT)
    for q in range(nq):
        row = score[q]
        idx = np.nonzero(row.astype(np.int64) >= min_score)[0]
        order = idx[np.lexsort((idx, -row[idx].astype(np.int64)))][:k]
        n = len(order)
        n_hits[q] = n
        hits[q, :n]["target"], hits[q, :n]["score"] = order, row[order]
        if end_a is not None:
            hits[q, :n]["end_a"], hits[q, :n]["end_b"] = end_a[q, order], end_b[q, order]
    return n_hits, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--no-cross", action="store_true", help="skip the matrix call and the host top-k")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    with S.Context(0) as ctx:
        for name, make, spec, is_sw, k, min_score in workloads():
            if only and name not in only:
                continue
            q, t = make()
            sc = S.make_scoring(spec)
            fn = ctx.sw_score_search if is_sw else ctx.nw_score_search
            ms, (n_hits, hits) = median_ms(lambda: fn(q, t, sc, k, min_score=min_score), args.calls, args.warm)
            launches = {kk: v[0] for kk, v in ctx.last_call().items()}
            n = cells(q, t)
            line = {
                "workload": name, "mode": "sw" if is_sw else "nw", "queries": q.n_seqs, "targets": t.n_seqs, "k": k,
                "min_score": min_score, "pairs": q.n_seqs * t.n_seqs, "cells": n, "call_ms": round(ms, 3),
                "gcups": round(n / (ms * 1e-3) / 1e9, 1),
                "h2d_bytes": int(q.len.sum(dtype=np.int64)) + int(t.len.sum(dtype=np.int64)) + 16 * (q.n_seqs + t.n_seqs),
                "d2h_bytes": q.n_seqs * (k * 16 + 4) + 16 * launches.get("score_select", 0),
                "cross_d2h_bytes": q.n_seqs * t.n_seqs * (12 if is_sw else 4), "launches": launches,
                "hits_mean": round(float(n_hits.mean()), 2)}
            if not args.no_cross:
                def cross():
                    if is_sw:
                        return ctx.sw_score_cross(q, t, sc)
                    return ctx.nw_score_cross(q, t, sc), None, None
                cross_ms, dense = median_ms(cross, args.calls, args.warm)
                t0 = time.perf_counter()
                want = host_top_k(*dense, k, min_score)
                line["cross_call_ms"] = round(cross_ms, 3)
                line["host_topk_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                line["cross_plus_topk_ms"] = round(line["cross_call_ms"] + line["host_topk_ms"], 3)
                line["identical"] = bool(np.array_equal(want[0], n_hits) and all(
                    np.array_equal(want[1][i, :c], hits[i, :c]) for i, c in enumerate(n_hits.tolist())))
                del dense
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
