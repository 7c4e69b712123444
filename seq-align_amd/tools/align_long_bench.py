#!/usr/bin/env python3
"""align_long_bench.py -- alignments of pairs of any size (seqalign_nw_align_long / seqalign_sw_align_long) against the calls they
are measured with, in one process.

Workloads (seeded, default DNA-style scorings):
  L1   1 NW 100 000 x 100 000, b = a with 10 % edits           against nw_score on the same pair   (target: call <= 4x)
  L2   1 NW 40 000 x 40 000 (under the 2^31-cell cap), 10 %     against nw_batch on the same pair   (recorded)
  L3   1 SW 60 000 x 60 000, a 3 000-long segment planted       against sw_score on the same pair   (target: call <= 2x)
  L4   16 NW 5 000 x 5 000, 10 % edits                          against nw_batch                    (recorded)

One JSON line per workload:
  call_ms, base_ms   median wall clock of the synchronous call and of the one it is measured with (3 calls after a warm-up
                     each); ratio = call_ms / base_ms
  rows_per_block, blocks, checkpoints   the plan the call ran (R: rows per block; blocks: long_block launches, per call)
  ckpt_bytes, block_bytes               device memory of the pair's checkpoints and of its block (sa_batch_long.hip)
  identical          NW: the score equals nw_score's (L1), the whole result nw_batch's (L2, L4); SW (L3): score and
                     end equal sw_score's
Kernel times per kind: a run of its own under `rocprofv3 --kernel-trace --stats`.

    python seq-align_amd/tools/align_long_bench.py [--only L1,L3] [--calls 3] [--warm 1]
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

NW_SPEC = {"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]}
SW_SPEC = {"init": [2, -3, -60, -2, 0, 0, 0, 0, 0, 0]}


def related(rng, n, edits):
    """a random DNA sequence of n and a copy with about `edits` of its positions substituted, deleted or followed by an
    insertion (tests/test_gpu_align_long.py: related)"""
    al = np.frombuffer(b"ACGT", np.uint8)
    a = al[rng.below(4, n).astype(np.int64)]
    kind = rng.below(1000, n).astype(np.int64)
    subs = al[rng.below(4, n).astype(np.int64)]
    cut = int(edits * 1000)
    out = bytearray()
    for i in range(n):
        k = kind[i]
        if k < cut // 3:
            out.append(int(subs[i]))
        elif k < 2 * cut // 3:
            continue
        else:
            out.append(int(a[i]))
            if k < cut:
                out.append(int(subs[i]))
    return a.tobytes(), bytes(out)


def planted(rng, n, seg_len, oa, ob):
    seg = np.frombuffer(b"ACGT", np.uint8)[rng.below(4, seg_len).astype(np.int64)].tobytes()
    bg_a = np.frombuffer(b"AC", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
    bg_b = np.frombuffer(b"GT", np.uint8)[rng.below(2, n).astype(np.int64)].tobytes()
    return bg_a[:oa] + seg + bg_a[oa + seg_len:], bg_b[:ob] + seg + bg_b[ob + seg_len:]


def plan(la, lb):
    """the rows per block of the default plan when the budget does not bind (sa_batch_long.hip: choose_plan)"""
    C = la + 1
    R = max(1, min(lb, ((1 << 31) - 1) // C - 1))
    nck = (lb - 1) // R if lb else 0
    return R, nck, 12 * C * nck, 12 * C * (min(R, lb) + 1)


def median_ms(fn, calls, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="L1,L2,L3,L4")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    args = ap.parse_args()
    only = set(args.only.split(","))
    nw, sw = S.make_scoring(NW_SPEC), S.make_scoring(SW_SPEC)
    with S.Context(0) as ctx:
        for name in ("L1", "L2", "L3", "L4"):
            if name not in only:
                continue
            rng = W.Rng(1000 + int(name[1]))
            if name == "L1":
                batch = W.from_pairs([related(rng, 100_000, 0.10)])
            elif name == "L2":
                batch = W.from_pairs([related(rng, 40_000, 0.10)])
            elif name == "L3":
                batch = W.from_pairs([planted(rng, 60_000, 3000, 21111, 38888)])
            else:
                batch = W.from_pairs([related(rng, 5000, 0.10) for _ in range(16)])
            if name == "L3":
                call = lambda: ctx.sw_align_long(batch, sw, 1)
                base = lambda: ctx.sw_score(batch, sw)
                base_name = "sw_score"
            else:
                call = lambda: ctx.nw_align_long(batch, nw)
                base = (lambda: ctx.nw_score(batch, nw)) if name == "L1" else (lambda: ctx.nw_batch(batch, nw))
                base_name = "nw_score" if name == "L1" else "nw_batch"
            call_ms, call_all = median_ms(call, args.calls, args.warm)
            got = call()
            info = ctx.last_call()
            base_ms, base_all = median_ms(base, args.calls, args.warm)
            want = base()
            if name == "L3":
                h = got[0][0]
                s, ea, eb = want
                identical = (h["score"], h["pos_a"] + h["len_a"], h["pos_b"] + h["len_b"]) == (int(s[0]), int(ea[0]), int(eb[0]))
            elif name == "L1":
                identical = [g[0] for g in got] == [int(v) for v in want]
            else:
                identical = got == want
            la, lb = int(batch.len_a[0]), int(batch.len_b[0])
            R, nck, ck_bytes, blk_bytes = plan(la, lb)
            print(json.dumps({
                "workload": name, "pairs": batch.n_pairs, "len_a": la, "len_b": lb, "cells": batch.n_pairs * la * lb,
                "call_ms": round(call_ms, 2), "call_ms_all": [round(x, 2) for x in call_all],
                "base": base_name, "base_ms": round(base_ms, 2), "base_ms_all": [round(x, 2) for x in base_all],
                "ratio": round(call_ms / base_ms, 3),
                "rows_per_block": R, "checkpoints": nck, "ckpt_bytes": ck_bytes, "block_bytes": blk_bytes,
                "blocks": info.get("long_block", (0, 0))[0], "launches": {k: v[0] for k, v in info.items()},
                "identical": bool(identical)}), flush=True)


if __name__ == "__main__":
    main()
