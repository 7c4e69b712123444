#!/usr/bin/env python3
"""nw_stats_banded_bench.py -- the banded NW statistics call (seqalign_nw_stats_banded) next to the banded NW score kernel, the
banded SW statistics kernel on the same diagonals, the banded alignment call plus a host count of its strings (the route it
replaces) and the unbanded statistics call, on the same batch, in one process.

Workloads (seeded, scoring 1 / -2 / -4 / -1, 8 % edits in equal thirds; align_banded_bench.py's generator):
  a   10 000 pairs of about 700 bp, w = 32   (65 to about 95 diagonals by the pair's difference in length: 2 per lane)
  b   1 000 pairs of about 10 kb, w = 255    (511 and 512 diagonals: 8 per lane.  The cap of 512 leaves room for lengths 0 or
      1 apart at this w, so seq_b is cut, or lengthened with random letters, to len_a or len_a + 1 -- one more edit at its end)

One JSON line per workload.  *_kernel_ms: {"median", "min", "max"} of --repeats launches between HIP events after a warm-up
(seqalign_nw_stats_band_time_ms, seqalign_band_score_time_ms, seqalign_sw_stats_band_time_ms with diag_lo / diag_hi set to each
pair's d_lo / d_hi; the batch uploaded once).  *_call_ms: the same of --calls whole calls (wall clock: host arrays in, host
arrays out):
  stats_banded_*          seqalign_nw_stats_banded
  score_banded_*          seqalign_nw_score_banded
  sw_stats_banded_*       seqalign_sw_stats_banded on the same diagonals
  align_count_call_ms     seqalign_nw_align_banded plus counting the columns of its strings on the host
  stats_call_ms           the unbanded seqalign_nw_stats_batch
Aims, set before anything ran and recorded as met or missed:
  aim_kernel              stats_banded_kernel_ms <= sw_stats_banded_kernel_ms (medians of this process; the margin over several
                          processes is the reader's: profiles/r24)
  aim_call_met            stats_banded_call_ms < align_count_call_ms and < stats_call_ms (medians)
Before a line is printed the tool ASSERTS that the scores are seqalign_nw_score_banded's bit for bit and that all three outputs
equal the alignment call's score and its counted strings for every pair; it exits non-zero otherwise.

    python seq-align_amd/tools/nw_stats_banded_bench.py [--only a,b] [--repeats 20] [--calls 10] [--scale 1]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python"), str(ROOT / "seq-align_amd" / "tools")]

import seqalign_amd as S                                                  # noqa: E402
from seqalign_amd import workloads as W                                   # noqa: E402
from align_banded_bench import NW_SPEC, band_of, related                  # noqa: E402
from nw_stats_bench import count_columns                                  # noqa: E402
from sw_stats_bench import spread, timed                                  # noqa: E402

WORKLOADS = {"a": (10_000, 700, 32), "b": (1_000, 10_000, 255)}           # pairs, letters, w
MAX_WIDTH = 512


def workload(name, scale):
    """(batch, w, d_lo[n], d_hi[n])"""
    n, letters, w = WORKLOADS[name]
    rng = W.Rng(2400 + sum(name.encode()))
    pairs = []
    for k in range(max(1, n // scale)):
        a, b = related(rng, letters, 0.08)
        if name == "b":
            b = (b + related(rng, 200, 0.0)[0])[:len(a) + k % 2]
        pairs.append((a, b))
    bands = [band_of(len(a), len(b), w) for a, b in pairs]
    assert all(hi - lo + 1 <= MAX_WIDTH for lo, hi in bands)
    return W.from_pairs(pairs), w, np.array([lo for lo, _ in bands], np.int32), np.array([hi for _, hi in bands], np.int32)


def run_workload(ctx, sc, name, args):
    batch, w, lo, hi = workload(name, args.scale)
    n = batch.n_pairs
    width = (hi.astype(np.int64) - lo + 1)
    cells = int(((batch.len_b.astype(np.int64) + 1) * width).sum())

    def align_and_count():
        return [(score,) + count_columns(sc, ra, rb) for score, ra, rb in ctx.nw_align_banded(batch, sc, w)]

    # results first: against the score call and the align call's counted strings
    got = ctx.nw_stats_banded(batch, sc, w)
    launches = ctx.last_call()
    assert np.array_equal(got[0], ctx.nw_score_banded(batch, sc, w)), (name, "the scores differ from nw_score_banded's")
    want = align_and_count()
    wrong = [p for p in range(n) if tuple(int(x[p]) for x in got) != want[p]]
    assert not wrong, (name, "the statistics call differs from the align call's score and its counted strings", wrong[:5])
    m, mm = got[1].astype(np.int64), got[2].astype(np.int64)
    length = batch.len_a.astype(np.int64) + batch.len_b - m - mm

    repeats, calls = args.repeats, args.calls
    out = {"workload": name, "pairs": n, "w": w, "min_width": int(width.min()), "max_width": int(width.max()), "band_cells": cells,
           "cells": batch.cells(), "timed_launches": int(repeats), "timed_calls": int(calls),
           "identity_mean": round(float(np.mean(m / np.maximum(1, length))), 4)}
    ctx.nw_stats_band_time_ms(batch, sc, w, 2)                            # warm-up
    out["stats_banded_kernel_ms"] = spread(ctx.nw_stats_band_time_ms(batch, sc, w, repeats))
    ctx.band_score_time_ms(batch, sc, w, 2)
    out["score_banded_kernel_ms"] = spread(ctx.band_score_time_ms(batch, sc, w, repeats))
    ctx.sw_stats_band_time_ms(batch, sc, lo, hi, 2)
    out["sw_stats_banded_kernel_ms"] = spread(ctx.sw_stats_band_time_ms(batch, sc, lo, hi, repeats))
    out["stats_over_sw_stats_kernel"] = round(out["stats_banded_kernel_ms"]["median"] / out["sw_stats_banded_kernel_ms"]["median"], 3)
    out["stats_over_score_kernel"] = round(out["stats_banded_kernel_ms"]["median"] / out["score_banded_kernel_ms"]["median"], 3)
    out["stats_banded_band_gcups"] = round(cells / (out["stats_banded_kernel_ms"]["median"] * 1e-3) / 1e9, 1)
    out["stats_banded_call_ms"] = timed(lambda: ctx.nw_stats_banded(batch, sc, w), calls)
    out["score_banded_call_ms"] = timed(lambda: ctx.nw_score_banded(batch, sc, w), calls)
    out["sw_stats_banded_call_ms"] = timed(lambda: ctx.sw_stats_banded(batch, sc, lo, hi), calls)
    out["align_count_call_ms"] = timed(align_and_count, calls)
    out["stats_call_ms"] = timed(lambda: ctx.nw_stats(batch, sc), calls)
    out["align_count_over_stats_banded_call"] = round(out["align_count_call_ms"]["median"] / out["stats_banded_call_ms"]["median"], 2)
    out["stats_over_stats_banded_call"] = round(out["stats_call_ms"]["median"] / out["stats_banded_call_ms"]["median"], 2)
    out["equals_score_call"] = out["equals_align_count"] = True
    out["launches"] = {k: v[0] for k, v in launches.items()}
    out["aim_kernel"] = "met" if out["stats_banded_kernel_ms"]["median"] <= out["sw_stats_banded_kernel_ms"]["median"] else "missed"
    out["aim_call_met"] = bool(out["stats_banded_call_ms"]["median"] < min(out["align_count_call_ms"]["median"], out["stats_call_ms"]["median"]))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the pair counts (a quick run)")
    args = ap.parse_args()
    sc = S.make_scoring(NW_SPEC)
    with S.Context(0) as ctx:
        outs = [run_workload(ctx, sc, name, args) for name in args.only.split(",") if name]
    for out in outs:
        if out["aim_kernel"] != "met":
            print(f"workload {out['workload']}: the NW statistics kernel's median is above the SW statistics kernel's in this process", file=sys.stderr, flush=True)
        if not out["aim_call_met"]:
            print(f"workload {out['workload']}: AIM MISSED: the call is not faster than align + count and the unbanded call", file=sys.stderr, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
