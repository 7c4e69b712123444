#!/usr/bin/env python3
"""score_cross_bench.py -- the score-matrix calls (seqalign_nw_score_cross / seqalign_sw_score_cross), and the pairwise
score call on the same pairs, in one process.

Workloads (seeded):
  X1   all-vs-all SW, BLOSUM62: 2 000 proteins of length 100-500 against themselves
  X2   NW, default DNA scoring: 1 000 reads of 150 against 10 000 reads of 150
  X3   NW: 16 queries of 3 000 against 64 targets of 3 000 (queries over 1 024 columns: the strips)
  cmp  X1's first 500 queries against its 2 000 targets, through sw_score_cross and through sw_score (seqalign_sw_score_batch)
       on the materialised batch

One JSON line per workload:
  call_ms     median wall clock of the synchronous call (host arrays in, matrices out), after `--warm` calls
  gcups       len_a x len_b cells / call_ms
  h2d_bytes   what the call sends to the device, from its layout: sequences and descriptors (cross: each set's bytes once per
              tile, 16 B per sequence; batch: len_a + len_b and 32 B of descriptors per pair)
  launches    what the call launched (seqalign_ctx_last_call_info)
Kernel times: a run of its own under `rocprofv3 --kernel-trace --stats` (the cross kernels are score_rows_kernel<..., true>,
the pairwise call's score_rows_kernel<..., false>); per call = total / (calls + warm).

    python seq-align_amd/tools/score_cross_bench.py [--only X1,cmp] [--calls 5] [--warm 1]
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


def fixed_set(n, length, seed):
    return W.random_set(n, seed, length, length, DNA)


def workloads():
    blosum, dna = {"preset": "BLOSUM62"}, {"preset": "default"}
    proteins = W.random_set(2000, 1, 100, 500, PROTEIN)
    yield "X1", lambda: (proteins, proteins), blosum, 1
    yield "X2", lambda: (fixed_set(1000, 150, 2), fixed_set(10000, 150, 3)), dna, 0
    yield "X3", lambda: (fixed_set(16, 3000, 4), fixed_set(64, 3000, 5)), dna, 0


def cells(q, t):
    return int(q.len.astype(np.int64).sum()) * int(t.len.astype(np.int64).sum())


def cross_h2d_bytes(q, t):   # one tile (the default budget holds every workload here)
    return int(q.len.sum(dtype=np.int64)) + int(t.len.sum(dtype=np.int64)) + 16 * (q.n_seqs + t.n_seqs)


def batch_h2d_bytes(b):
    return int(b.len_a.sum(dtype=np.int64)) + int(b.len_b.sum(dtype=np.int64)) + 32 * b.n_pairs


def median_ms(fn, calls, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def cross_call(ctx, q, t, sc, is_sw):
    return (lambda: ctx.sw_score_cross(q, t, sc)) if is_sw else (lambda: ctx.nw_score_cross(q, t, sc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    with S.Context(0) as ctx:
        for name, make, spec, is_sw in workloads():
            if only and name not in only:
                continue
            q, t = make()
            sc = S.make_scoring(spec)
            ms, ms_min = median_ms(cross_call(ctx, q, t, sc, is_sw), args.calls, args.warm)
            n = cells(q, t)
            print(json.dumps({
                "workload": name, "mode": "sw" if is_sw else "nw", "queries": q.n_seqs, "targets": t.n_seqs,
                "pairs": q.n_seqs * t.n_seqs, "cells": n, "call_ms": round(ms, 3), "call_ms_min": round(ms_min, 3),
                "gcups": round(n / (ms * 1e-3) / 1e9, 1), "h2d_bytes": cross_h2d_bytes(q, t),
                "launches": {k: v[0] for k, v in ctx.last_call().items()}}), flush=True)
        if not only or "cmp" in only:
            proteins = W.random_set(2000, 1, 100, 500, PROTEIN)
            q = W.SeqSet(proteins.arena, proteins.off[:500].copy(), proteins.len[:500].copy())
            sc = S.make_scoring({"preset": "BLOSUM62"})
            batch = W.cross_batch(q, proteins)
            n = cells(q, proteins)
            cross_ms, _ = median_ms(cross_call(ctx, q, proteins, sc, 1), args.calls, args.warm)
            cross_launches = {k: v[0] for k, v in ctx.last_call().items()}
            batch_ms, _ = median_ms(lambda: ctx.sw_score(batch, sc), args.calls, args.warm)
            batch_launches = {k: v[0] for k, v in ctx.last_call().items()}
            got, want = ctx.sw_score_cross(q, proteins, sc), ctx.sw_score(batch, sc)
            same = all(np.array_equal(g, w.reshape(g.shape)) for g, w in zip(got, want))
            print(json.dumps({
                "workload": "cmp", "mode": "sw", "queries": q.n_seqs, "targets": proteins.n_seqs, "pairs": batch.n_pairs,
                "cells": n, "cross_call_ms": round(cross_ms, 3), "batch_call_ms": round(batch_ms, 3),
                "cross_gcups": round(n / (cross_ms * 1e-3) / 1e9, 1), "batch_gcups": round(n / (batch_ms * 1e-3) / 1e9, 1),
                "batch_over_cross": round(batch_ms / cross_ms, 3), "cross_h2d_bytes": cross_h2d_bytes(q, proteins),
                "batch_h2d_bytes": batch_h2d_bytes(batch), "identical": same,
                "cross_launches": cross_launches, "batch_launches": batch_launches}), flush=True)


if __name__ == "__main__":
    main()
