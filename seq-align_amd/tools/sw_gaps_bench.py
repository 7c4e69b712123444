#!/usr/bin/env python3
"""sw_gaps_bench.py -- the SW gap-run calls (seqalign_sw_gaps_batch / _banded / _banded_wide) next to the sw_counts call of the
same geometry on the same batch in the same process, one workload per process (profiles/r33).

Workloads (sw_counts_bench.py's nine):
  c3       10 000 reads of 150 bp in 400 bp windows                        unbanded; and sw_batch + a host count of '-' runs
  c4       4 000 pairs of 300 x 300 aa, BLOSUM62                           unbanded
  reads    10 000 reads of 700 bp in 1 000 bp windows (two strips)         unbanded
  long     64 related pairs of 5 000 x 5 000                               unbanded
  one      one related pair of 60 000 x 60 000                             unbanded
  n32      10 000 reads in their windows, the read's diagonal +- 32        narrow banded
  n255     1 000 reads of 10 kb, +- 255                                    narrow banded
  w1024    1 000 reads of 10 kb in 14 kb windows, +- 1 024                 wide banded; and sw_align_banded_wide + a host count
  w2048    16 reads of 200 kb with 8 % edits in 210 kb windows, +- 2 048   wide banded

One JSON line.  *_kernel_ms: {"median", "min", "max"} of --launches launches between HIP events (the time hooks; the wide calls
have none: their *_call_ms stand in).  *_call_ms: the same of --calls whole calls (wall clock).  Before the line is printed the
tool ASSERTS that score and end are the score call's byte for byte and, on c3 and w1024, that the two run counts are those of
the align call's strings counted on the host.
Aims, set before anything ran (the margin over several processes is the reader's: the larger of the two kernels' own max - min
over the processes, profiles/r23's rule):
  aim1   gaps within that margin of the sw_counts sibling, on the kernel medians where there is a time hook.  The tool cannot
         judge it: a process knows its own spread only.  "one_process_compare" is sw_stats_bench.verdict on this process alone
         (level where each median lies in the other's spread) and is NOT the aim's outcome
  aim2   c3: the gaps call is faster than sw_batch(min_score = 1, max_hits = 1) plus a host count of '-' runs;
         w1024: faster than sw_align_banded_wide(min_score = 1) plus that count

    python seq-align_amd/tools/sw_gaps_bench.py --workload c3 [--launches 20] [--calls 10] [--scale 1]
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
import align_banded_wide_bench as WB                                      # noqa: E402
from sw_counts_bench import UNBANDED, WORKLOADS, long_reads, same_bytes   # noqa: E402
from sw_span_banded_bench import bounds                                   # noqa: E402
from sw_stats_bench import batch_of, spread, timed, verdict               # noqa: E402


def runs_of(text) -> int:
    """Maximal runs of '-' in one string of a hit."""
    return sum(1 for k, ch in enumerate(text) if ch == "-" and (k == 0 or text[k - 1] != "-"))


def host_runs(hits_per_pair):
    """(gap_runs_a, gap_runs_b) arrays from the align calls' hit lists, at most one hit per pair."""
    ga = np.array([runs_of(h[0]["a"]) if h else 0 for h in hits_per_pair], np.uint32)
    gb = np.array([runs_of(h[0]["b"]) if h else 0 for h in hits_per_pair], np.uint32)
    return ga, gb


def run(ctx, name, args):
    out = {"workload": name, "launches": args.launches, "calls": args.calls}
    if name in UNBANDED:
        spec, batch = batch_of(name, args.scale)
        sc = S.make_scoring(spec)
        got = ctx.sw_gaps(batch, sc)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert same_bytes(got[:3], ctx.sw_score(batch, sc)), "score and end differ from sw_score's"
        out["gaps_kernel_ms"] = spread(ctx.sw_gaps_time_ms(batch, sc, repeats=args.launches))
        out["counts_kernel_ms"] = spread(ctx.sw_counts_time_ms(batch, sc, repeats=args.launches))
        out["gaps_call_ms"] = timed(lambda: ctx.sw_gaps(batch, sc), args.calls)
        out["counts_call_ms"] = timed(lambda: ctx.sw_counts(batch, sc), args.calls)
        if name == "c3":
            def align_and_count():
                return host_runs(ctx.sw_batch(batch, sc, 1, 1))

            ga, gb = align_and_count()
            assert np.array_equal(ga, got[3]) and np.array_equal(gb, got[4]), "the runs differ from sw_batch's strings"
            out["align_count_call_ms"] = timed(align_and_count, max(2, args.calls // 2))
            out["aim2"] = "met" if out["gaps_call_ms"]["median"] < out["align_count_call_ms"]["median"] else "missed"
    elif name in ("n32", "n255"):
        sc = S.make_scoring(WB.SW_SPEC)
        batch, lo, hi = bounds("a" if name == "n32" else "b", args.scale)
        got = ctx.sw_gaps_banded(batch, sc, lo, hi)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert same_bytes(got[:3], ctx.sw_score_banded(batch, sc, lo, hi)), "score and end differ from sw_score_banded's"
        out["gaps_kernel_ms"] = spread(ctx.sw_gaps_band_time_ms(batch, sc, lo, hi, repeats=args.launches))
        out["counts_kernel_ms"] = spread(ctx.sw_counts_band_time_ms(batch, sc, lo, hi, repeats=args.launches))
        out["gaps_call_ms"] = timed(lambda: ctx.sw_gaps_banded(batch, sc, lo, hi), args.calls)
        out["counts_call_ms"] = timed(lambda: ctx.sw_counts_banded(batch, sc, lo, hi), args.calls)
    else:
        sc = S.make_scoring(WB.SW_SPEC)
        if name == "w1024":
            batch, (lo, hi) = WB.workload("W4", args.scale)
            lo, hi = np.asarray(lo, np.int32), np.asarray(hi, np.int32)
        else:
            batch, lo, hi = long_reads(args.scale)
        got = ctx.sw_gaps_banded_wide(batch, sc, lo, hi)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert same_bytes(got[:3], ctx.sw_score_banded_wide(batch, sc, lo, hi)), "score and end differ from sw_score_banded_wide's"
        out["gaps_call_ms"] = timed(lambda: ctx.sw_gaps_banded_wide(batch, sc, lo, hi), args.calls)
        out["counts_call_ms"] = timed(lambda: ctx.sw_counts_banded_wide(batch, sc, lo, hi), args.calls)
        if name == "w1024":
            def align_and_count():
                return host_runs(ctx.sw_align_banded_wide(batch, sc, lo, hi, 1))

            ga, gb = align_and_count()
            assert np.array_equal(ga, got[3]) and np.array_equal(gb, got[4]), "the runs differ from sw_align_banded_wide's strings"
            out["align_count_call_ms"] = timed(align_and_count, max(2, args.calls // 5))
            out["aim2"] = "met" if out["gaps_call_ms"]["median"] < out["align_count_call_ms"]["median"] else "missed"
    out["pairs"] = batch.n_pairs
    out["gapopen_mean"] = round(float(np.mean(got[3].astype(np.int64) + got[4])), 3)
    ours = out.get("gaps_kernel_ms") or out["gaps_call_ms"]
    theirs = out.get("counts_kernel_ms") or out["counts_call_ms"]
    out["yardstick"] = "counts_kernel" if "counts_kernel_ms" in out else "counts_call"
    out["gaps_over_yardstick"] = round(ours["median"] / theirs["median"], 3)
    out["one_process_compare"] = verdict(ours, theirs)   # level / met / missed of THIS process alone; aim 1 is judged over three
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
