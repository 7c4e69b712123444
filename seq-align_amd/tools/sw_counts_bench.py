#!/usr/bin/env python3
"""sw_counts_bench.py -- the SW identity-count calls (seqalign_sw_counts_batch / _banded / _banded_wide) next to the sw_stats
call of the same geometry on the same batch in the same process, one workload per process (profiles/r32).

Workloads (sw_stats_bench.py's, sw_span_banded_bench.py's and align_banded_wide_bench.py's batches):
  c3       10 000 reads of 150 bp in 400 bp windows                        unbanded
  c4       4 000 pairs of 300 x 300 aa, BLOSUM62                           unbanded
  reads    10 000 reads of 700 bp in 1 000 bp windows (two strips)         unbanded
  long     64 related pairs of 5 000 x 5 000                               unbanded
  one      one related pair of 60 000 x 60 000                             unbanded
  n32      10 000 reads in their windows, the read's diagonal +- 32        narrow banded
  n255     1 000 reads of 10 kb, +- 255                                    narrow banded
  w1024    1 000 reads of 10 kb in 14 kb windows, +- 1 024                 wide banded; and sw_align_banded_wide + a host count
  w2048    16 reads of 200 kb with 8 % edits in 210 kb windows, +- 2 048   wide banded; sw_stats refuses: the yardstick is
                                                                           sw_span_banded_wide

One JSON line.  *_kernel_ms: {"median", "min", "max"} of --launches launches between HIP events (the time hooks; the wide calls
have none: their *_call_ms stand in).  *_call_ms: the same of --calls whole calls (wall clock).  Before the line is printed the
tool ASSERTS that score and end are the score call's byte for byte and that the counts are the sw_stats sibling's (the wide
workloads: that sw_span_banded_wide's pos + len is the end; w2048: that sw_stats_banded_wide refuses the batch).
Aims, set before anything ran (the margin over several processes is the reader's: the larger of the two kernels' own max - min
over the processes, profiles/r23's rule):
  aim1   counts <= the sw_stats sibling (w2048: the span sibling), on the kernel medians where there is a time hook
  aim2   w1024: the counts call is faster than sw_align_banded_wide(min_score = 1) plus a host count

    python seq-align_amd/tools/sw_counts_bench.py --workload c3 [--launches 20] [--calls 10] [--scale 1]
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
import align_banded_wide_bench as WB                                      # noqa: E402
from sw_span_banded_bench import bounds                                   # noqa: E402
from sw_stats_bench import batch_of, hit_fields, spread, timed, verdict   # noqa: E402

UNBANDED = ["c3", "c4", "reads", "long", "one"]
WORKLOADS = UNBANDED + ["n32", "n255", "w1024", "w2048"]


def long_reads(scale):
    """16 reads of 200 kb with 8 % edits in windows of 210 kb, the read's diagonal +- 2 048."""
    rng = W.Rng(3200)
    pairs, lo, hi = [], [], []
    for _ in range(max(1, 16 // scale)):
        window = WB.ACGT[rng.below(4, 210_000 // scale).astype(np.int64)]
        offset = int(rng.below(10_000 // scale + 1, 1)[0])
        _, read = WB.related_of(rng, window[offset:offset + 200_000 // scale], 0.08)
        pairs.append((read, window.tobytes()))
        lo.append(-offset - 2048)
        hi.append(-offset + 2048)
    return W.from_pairs(pairs), np.asarray(lo, np.int32), np.asarray(hi, np.int32)


def same_bytes(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def counts_of(stats):
    return [stats[0], stats[1] + stats[3], stats[2] + stats[4], stats[5], stats[6]]


def run(ctx, name, args):
    out = {"workload": name, "launches": args.launches, "calls": args.calls}
    if name in UNBANDED:
        spec, batch = batch_of(name, args.scale)
        sc = S.make_scoring(spec)
        got = ctx.sw_counts(batch, sc)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert same_bytes(got[:3], ctx.sw_score(batch, sc)), "score and end differ from sw_score's"
        assert same_bytes(got, counts_of(ctx.sw_stats(batch, sc))), "the counts differ from sw_stats'"
        out["counts_kernel_ms"] = spread(ctx.sw_counts_time_ms(batch, sc, repeats=args.launches))
        out["stats_kernel_ms"] = spread(ctx.sw_stats_time_ms(batch, sc, repeats=args.launches))
        out["span_kernel_ms"] = spread(ctx.sw_span_time_ms(batch, sc, repeats=args.launches))
        out["counts_call_ms"] = timed(lambda: ctx.sw_counts(batch, sc), args.calls)
        out["stats_call_ms"] = timed(lambda: ctx.sw_stats(batch, sc), args.calls)
    elif name in ("n32", "n255"):
        sc = S.make_scoring(WB.SW_SPEC)
        batch, lo, hi = bounds("a" if name == "n32" else "b", args.scale)
        got = ctx.sw_counts_banded(batch, sc, lo, hi)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert same_bytes(got[:3], ctx.sw_score_banded(batch, sc, lo, hi)), "score and end differ from sw_score_banded's"
        assert same_bytes(got, counts_of(ctx.sw_stats_banded(batch, sc, lo, hi))), "the counts differ from sw_stats_banded's"
        out["counts_kernel_ms"] = spread(ctx.sw_counts_band_time_ms(batch, sc, lo, hi, repeats=args.launches))
        out["stats_kernel_ms"] = spread(ctx.sw_stats_band_time_ms(batch, sc, lo, hi, repeats=args.launches))
        out["span_kernel_ms"] = spread(ctx.sw_span_band_time_ms(batch, sc, lo, hi, repeats=args.launches))
        out["counts_call_ms"] = timed(lambda: ctx.sw_counts_banded(batch, sc, lo, hi), args.calls)
        out["stats_call_ms"] = timed(lambda: ctx.sw_stats_banded(batch, sc, lo, hi), args.calls)
    else:
        sc = S.make_scoring(WB.SW_SPEC)
        if name == "w1024":
            batch, (lo, hi) = WB.workload("W4", args.scale)
            lo, hi = np.asarray(lo, np.int32), np.asarray(hi, np.int32)
        else:
            batch, lo, hi = long_reads(args.scale)
        got = ctx.sw_counts_banded_wide(batch, sc, lo, hi)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert same_bytes(got[:3], ctx.sw_score_banded_wide(batch, sc, lo, hi)), "score and end differ from sw_score_banded_wide's"
        span = ctx.sw_span_banded_wide(batch, sc, lo, hi)
        assert np.array_equal(span[1] + span[3], got[1]) and np.array_equal(span[2] + span[4], got[2]), "sw_span's pos + len is not the end"
        out["counts_call_ms"] = timed(lambda: ctx.sw_counts_banded_wide(batch, sc, lo, hi), args.calls)
        out["span_call_ms"] = timed(lambda: ctx.sw_span_banded_wide(batch, sc, lo, hi), args.calls)
        if name == "w1024":
            assert same_bytes(got, counts_of(ctx.sw_stats_banded_wide(batch, sc, lo, hi))), "the counts differ from sw_stats_banded_wide's"
            out["stats_call_ms"] = timed(lambda: ctx.sw_stats_banded_wide(batch, sc, lo, hi), args.calls)

            def align_and_count():
                return [hit_fields(sc, h) for h in ctx.sw_align_banded_wide(batch, sc, lo, hi, 1)]

            out["align_count_call_ms"] = timed(align_and_count, max(2, args.calls // 5))
            out["aim2"] = "met" if out["counts_call_ms"]["median"] < out["align_count_call_ms"]["median"] else "missed"
        else:
            try:                                       # (the align call would store 9.8 GB per pair here: no string check)
                ctx.sw_stats_banded_wide(batch, sc, lo, hi)
                out["stats_refuses"] = args.scale > 3
                assert args.scale > 3, "sw_stats_banded_wide took sequences over its limit"
            except S.SeqAlignError as e:
                assert e.code == S.E_TOO_LARGE, str(e)
                out["stats_refuses"] = True
    out["pairs"] = batch.n_pairs
    out["identity_mean"] = round(float(np.mean(got[3] / np.maximum(1, got[3].astype(np.int64) + got[4]))), 4)
    ours = out.get("counts_kernel_ms") or out["counts_call_ms"]
    theirs = out.get("stats_kernel_ms") or out.get("stats_call_ms") or out["span_call_ms"]
    out["yardstick"] = "stats_kernel" if "stats_kernel_ms" in out else "stats_call" if "stats_call_ms" in out else "span_call"
    out["counts_over_yardstick"] = round(ours["median"] / theirs["median"], 3)
    out["aim1"] = verdict(ours, theirs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=WORKLOADS)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the sizes (a quick run)")
    args = ap.parse_args()
    with S.Context(0) as ctx:
        out = run(ctx, args.workload, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
