#!/usr/bin/env python3
"""align_banded_bench.py -- banded NW (seqalign_nw_score_banded / seqalign_nw_align_banded) against the unbanded calls, in one
process.

Workloads (seeded, scoring 1 / -2 / -4 / -1, edits in equal thirds):
  B1   1 000 pairs x 10 000 bp, 8 % edits, w = 256      nw_align_banded against nw_batch, nw_score_banded against nw_score
  B2   10 000 pairs x 2 000 bp, 8 % edits, w = 64       the same
  B3   1 pair x 100 000 bp, 5 % edits, width <= 1 024   nw_align_banded against nw_align_long, nw_score_banded against nw_score
  B4   10 000 pairs x 150 bp, w = 16                    recorded only: small pairs belong to nw_batch.  The batch is C2's
       (bench.py, tests/golden/configs.json "C2": dna_nw_150, seed 1, UNRELATED pairs -- most paths leave a band of 16)
  F    frame rate, kernel time against kernel time (HIP events around the launches, sequences already on the device):
       seqalign_band_score_time_ms on pairs whose band fills a frame (64 x CPL - 1 diagonals) beside seqalign_score_time_ms
       on pairs as wide as that frame (len_a = 64 x CPL), same rows -- cells of the frame per second

One JSON line per workload: median wall clock of 3 synchronous calls after a warm-up.  Before a line is printed the tool
ASSERTS that the banded result equals the comparison call's for every pair whose path lies in the band (in_band counts them),
that no banded score is above the unbanded one and that the score call agrees with the align call; it exits non-zero
otherwise.  B1 / B2 carry `bar_met`: the banded call took less than half the comparison's time (a line with bar_met false
is flagged on stderr and the exit status is 2).  --scale divides the pair counts (a quick run).  Kernel times per kind: a run
of its own under `rocprofv3 --kernel-trace --stats`.

    python seq-align_amd/tools/align_banded_bench.py [--only B1,B3] [--scale 1] [--calls 3] [--warm 1]
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
ACGT = np.frombuffer(b"ACGT", np.uint8)


def related(rng, n, edits):
    """a random DNA sequence of n and a copy with about `edits` of its positions substituted, deleted or followed by an insertion"""
    a = ACGT[rng.below(4, n).astype(np.int64)]
    kind = rng.below(3000, n).astype(np.int64)
    subs = ACGT[rng.below(4, n).astype(np.int64)]
    cut = int(edits * 1000)
    counts = np.where(kind < cut, 0, np.where(kind < 2 * cut, 2, 1))
    base = np.where((kind >= 2 * cut) & (kind < 3 * cut), subs, a)
    out = np.repeat(base, counts)
    second = (np.cumsum(counts) - 1)[counts == 2]
    out[second] = subs[counts == 2]
    return a.tobytes(), out.tobytes()


def band_of(la, lb, w):
    return max(-lb, min(0, la - lb) - w), min(la, max(0, la - lb) + w)


def excursion(ra, rb):
    x, y = np.frombuffer(ra, np.uint8) != 0x2D, np.frombuffer(rb, np.uint8) != 0x2D
    d = np.cumsum(x.astype(np.int64) - y.astype(np.int64))
    return (min(0, int(d.min())), max(0, int(d.max()))) if len(d) else (0, 0)


def median_ms(fn, calls, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), [round(x, 2) for x in t]


def workload(name, scale):
    rng = W.Rng(1200 + sum(name.encode()))
    if name == "B1":
        return W.from_pairs([related(rng, 10_000, 0.08) for _ in range(max(1, 1000 // scale))]), 256
    if name == "B2":
        return W.from_pairs([related(rng, 2_000, 0.08) for _ in range(max(1, 10_000 // scale))]), 64
    if name == "B3":
        a, b = related(rng, 100_000, 0.05)
        return W.from_pairs([(a, b)]), (1024 - abs(len(a) - len(b)) - 1) // 2
    return W.dna_nw_150(max(1, 10_000 // scale), seed=1), 16


def run_workload(ctx, sc, name, args):
    batch, w = workload(name, args.scale)
    n = batch.n_pairs
    las, lbs = batch.len_a.astype(np.int64), batch.len_b.astype(np.int64)
    widths = [band_of(int(a), int(b), w)[1] - band_of(int(a), int(b), w)[0] + 1 for a, b in zip(las, lbs)]
    band_cells = int(sum((int(b) + 1) * wd for b, wd in zip(lbs, widths)))
    cells = int((las * lbs).sum())
    align_base = (lambda: ctx.nw_align_long(batch, sc)) if name == "B3" else (lambda: ctx.nw_batch(batch, sc))
    out = {"workload": name, "pairs": n, "w": w, "max_width": max(widths), "cells": cells, "band_cells": band_cells,
           "cell_ratio": round(cells / band_cells, 1)}
    ms, all_ = median_ms(lambda: ctx.nw_align_banded(batch, sc, w), args.calls, args.warm)
    got = ctx.nw_align_banded(batch, sc, w)
    out.update(align_banded_ms=round(ms, 2), align_banded_all=all_, align_launches=ctx.last_call())
    ms_b, all_b = median_ms(align_base, args.calls, args.warm)
    want = align_base()
    out.update(align_base="nw_align_long" if name == "B3" else "nw_batch", align_base_ms=round(ms_b, 2), align_base_all=all_b,
               align_base_launches=ctx.last_call(), align_speedup=round(ms_b / ms, 2))
    inside = []
    for p in range(n):
        lo, hi = excursion(want[p][1], want[p][2])
        d_lo, d_hi = band_of(int(las[p]), int(lbs[p]), w)
        inside.append(d_lo <= lo and hi <= d_hi)
    wrong = [p for p in range(n) if inside[p] and got[p] != want[p]]
    assert not wrong, (name, "banded result differs from the comparison call's although its path lies in the band", wrong[:5])
    above = [p for p in range(n) if got[p][0] > want[p][0]]
    assert not above, (name, "banded score above the unbanded one", above[:5])
    out.update(in_band=int(sum(inside)), identical=True, outside_not_above=True)
    ms, all_ = median_ms(lambda: ctx.nw_score_banded(batch, sc, w), args.calls, args.warm)
    ms_b, all_b = median_ms(lambda: ctx.nw_score(batch, sc), args.calls, args.warm)
    score = ctx.nw_score_banded(batch, sc, w)
    assert [int(s) for s in score] == [g[0] for g in got], (name, "the score call disagrees with the align call")
    out.update(score_banded_ms=round(ms, 2), score_banded_all=all_, score_base="nw_score", score_base_ms=round(ms_b, 2),
               score_base_all=all_b, score_speedup=round(ms_b / ms, 2), score_equals_align=True)
    ok = True
    if name in ("B1", "B2"):
        ok = out["align_speedup"] > 2 and out["score_speedup"] > 2
        out["bar_met"] = ok
    elif name == "B3":
        ok = out["align_speedup"] > 1
        out["bar_met"] = ok
    print(json.dumps(out), flush=True)
    if not ok:
        print(f"{name}: BAR MISSED: align {out['align_speedup']}x, score {out['score_speedup']}x", file=sys.stderr, flush=True)
    return ok


def run_frame_rate(ctx, sc, args):
    rows, pairs = 4000, max(64, 4096 // args.scale)
    rng = W.Rng(77)
    for cpl in (1, 2, 4, 8, 16):
        frame = 64 * cpl
        seqs = [related(rng, rows, 0.02) for _ in range(8)]
        # equal lengths: width = 1 + 2 w is odd, so the band fills the frame to 64 x CPL - 1 diagonals
        batch = W.from_pairs([(seqs[k % 8][0], seqs[k % 8][0]) for k in range(pairs)])
        w = (frame - 1) // 2
        band_ms = float(np.median(ctx.band_score_time_ms(batch, sc, w, repeats=5)))
        wide = W.from_pairs([(seqs[k % 8][0][:frame], seqs[k % 8][1][:rows]) for k in range(pairs)])
        full_ms = float(np.median(ctx.score_time_ms(wide, sc, 0, repeats=5)))
        band_rate = pairs * rows * frame / (band_ms * 1e-3)
        full_rate = pairs * int(wide.len_b[0]) * frame / (full_ms * 1e-3)
        print(json.dumps({"workload": "F", "cpl": cpl, "pairs": pairs, "rows": rows, "band_width": 2 * w + 1,
                          "band_kernel_ms": round(band_ms, 3), "band_frame_cells_per_s": round(band_rate, 0),
                          "score_rows_rows": int(wide.len_b[0]), "score_rows_kernel_ms": round(full_ms, 3),
                          "score_rows_frame_cells_per_s": round(full_rate, 0),
                          "moving_frame_cost": round(full_rate / band_rate, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="B1,B2,B3,B4,F")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    args = ap.parse_args()
    only = set(args.only.split(","))
    sc = S.make_scoring(NW_SPEC)
    with S.Context(0) as ctx:
        ok = True
        for name in ("B1", "B2", "B3", "B4"):
            if name in only:
                ok = run_workload(ctx, sc, name, args) and ok
        if "F" in only:
            run_frame_rate(ctx, sc, args)
    if not ok:
        sys.exit(2)


if __name__ == "__main__":
    main()
