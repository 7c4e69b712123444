#!/usr/bin/env python3
"""nw_gaps_bench.py -- the NW gap-run calls (seqalign_nw_gaps_batch / _cross / _banded / _banded_wide) next to the nw_stats call
of the same geometry on the same batch in the same process, one workload per process (profiles/r34).

Workloads:
  c2       10 000 pairs of 150 x 150 DNA                                    unbanded; and nw_batch + a host count of '-' runs
  b62      4 000 pairs of 300 x 300 aa, BLOSUM62                            unbanded
  long     64 related pairs of 5 000 x 5 000                                unbanded
  one      one related pair of 60 000 x 60 000                              unbanded
  n32      1 000 related pairs of 10 kb, w = 32                             narrow banded
  n255     the same pairs, w = 255                                          narrow banded
  w1024    the same pairs, w = 1 024                                        wide banded; and nw_align_banded_wide + a host count
  w2048    4 related pairs of 200 kb with 8 % edits, w = 2 048              wide banded
  cross    64 protein queries x 4 000 targets of about 300 aa, BLOSUM62     nw_gaps_cross against nw_gaps on the explicit batch

One JSON line.  *_kernel_ms: {"median", "min", "max"} of --launches launches between HIP events (the time hooks; the wide and
cross calls have none: their *_call_ms stand in).  *_call_ms: the same of --calls whole calls (wall clock).  Before the line is
printed the tool ASSERTS that the score is the score call's byte for byte and, on c2 and w1024, that the two run counts are
those of the align call's strings counted on the host; on cross, that the matrices equal the explicit batch's result.
Aims, set before anything ran (the margin over several processes is the reader's: the larger of the two kernels' own max - min
over the processes, profiles/r23's rule):
  aim1   gaps within that margin of the nw_stats sibling, on the kernel medians where there is a time hook.  The tool cannot
         judge it: a process knows its own spread only.  "one_process_compare" is sw_stats_bench.verdict on this process alone
         and is NOT the aim's outcome
  aim2   c2: the gaps call is faster than nw_batch plus a host count of '-' runs;
         w1024: faster than nw_align_banded_wide plus that count
  aim3   cross: nw_gaps_cross no slower than nw_gaps on the explicit batch (call medians)

    python seq-align_amd/tools/nw_gaps_bench.py --workload c2 [--launches 20] [--calls 10] [--scale 1]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python"), str(ROOT / "seq-align_amd" / "tools")]

import seqalign_amd as S                                                  # noqa: E402
from seqalign_amd import workloads as W                                   # noqa: E402
import align_banded_wide_bench as WB                                      # noqa: E402
import nw_stats_banded_bench as NB                                        # noqa: E402
from nw_stats_bench import batch_of                                       # noqa: E402
from sw_gaps_bench import runs_of                                         # noqa: E402
from sw_stats_bench import spread, timed, verdict                         # noqa: E402

UNBANDED = ["c2", "b62", "long", "one"]
NARROW = {"n32": 32, "n255": 255}
WORKLOADS = UNBANDED + list(NARROW) + ["w1024", "w2048", "cross"]


def host_runs(aligned):
    """(gap_runs_a, gap_runs_b) arrays from the align calls' (score, a, b) per pair."""
    ga = np.array([runs_of(ra.decode()) for _, ra, _ in aligned], np.uint32)
    gb = np.array([runs_of(rb.decode()) for _, _, rb in aligned], np.uint32)
    return ga, gb


def long_pairs(scale):
    rng = W.Rng(3400)
    return W.from_pairs([WB.related(rng, 200_000 // scale, 0.08) for _ in range(4)]), 2048


def run_cross(ctx, args):
    sc = S.make_scoring({"preset": "BLOSUM62"})
    q = W.random_set(max(1, 64 // args.scale), 401, 270, 330, bytes(W.AMINO20))
    t = W.random_set(max(1, 4000 // args.scale), 402, 270, 330, bytes(W.AMINO20))
    out = {"workload": "cross", "queries": q.n_seqs, "targets": t.n_seqs, "calls": args.calls}
    t0 = time.perf_counter()
    explicit = W.cross_batch(q, t)
    out["batch_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    got = ctx.nw_gaps_cross(q, t, sc)
    out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
    want = ctx.nw_gaps(explicit, sc)
    assert all(np.array_equal(g.ravel(), w) for g, w in zip(got, want)), "matrices differ from the explicit batch's result"
    assert got[0].tobytes() == ctx.nw_score_cross(q, t, sc).tobytes(), "scores differ from nw_score_cross"
    out["gaps_cross_call_ms"] = timed(lambda: ctx.nw_gaps_cross(q, t, sc), args.calls)
    out["gaps_batch_call_ms"] = timed(lambda: ctx.nw_gaps(explicit, sc), args.calls)
    out["stats_cross_call_ms"] = timed(lambda: ctx.nw_stats_cross(q, t, sc), args.calls)
    out["aim3"] = "met" if out["gaps_cross_call_ms"]["median"] <= out["gaps_batch_call_ms"]["median"] else "missed"
    out["gaps_over_stats_cross"] = round(out["gaps_cross_call_ms"]["median"] / out["stats_cross_call_ms"]["median"], 3)
    return out


def run(ctx, name, args):
    out = {"workload": name, "launches": args.launches, "calls": args.calls}
    if name in UNBANDED:
        spec, batch = batch_of(name, args.scale)
        sc = S.make_scoring(spec)
        got = ctx.nw_gaps(batch, sc)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert got[0].tobytes() == ctx.nw_score(batch, sc).tobytes(), "the score differs from nw_score's"
        out["gaps_kernel_ms"] = spread(ctx.nw_gaps_time_ms(batch, sc, repeats=args.launches))
        out["stats_kernel_ms"] = spread(ctx.nw_stats_time_ms(batch, sc, repeats=args.launches))
        out["gaps_call_ms"] = timed(lambda: ctx.nw_gaps(batch, sc), args.calls)
        out["stats_call_ms"] = timed(lambda: ctx.nw_stats(batch, sc), args.calls)
        if name == "c2":
            def align_and_count():
                return host_runs(ctx.nw_batch(batch, sc))

            ga, gb = align_and_count()
            assert np.array_equal(ga, got[1]) and np.array_equal(gb, got[2]), "the runs differ from nw_batch's strings"
            out["align_count_call_ms"] = timed(align_and_count, max(2, args.calls // 2))
            out["aim2"] = "met" if out["gaps_call_ms"]["median"] < out["align_count_call_ms"]["median"] else "missed"
    elif name in NARROW:
        sc = S.make_scoring(WB.NW_SPEC)
        batch, w = NB.workload("b", args.scale)[0], NARROW[name]
        got = ctx.nw_gaps_banded(batch, sc, w)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert got[0].tobytes() == ctx.nw_score_banded(batch, sc, w).tobytes(), "the score differs from nw_score_banded's"
        out["gaps_kernel_ms"] = spread(ctx.nw_gaps_band_time_ms(batch, sc, w, repeats=args.launches))
        out["stats_kernel_ms"] = spread(ctx.nw_stats_band_time_ms(batch, sc, w, repeats=args.launches))
        out["gaps_call_ms"] = timed(lambda: ctx.nw_gaps_banded(batch, sc, w), args.calls)
        out["stats_call_ms"] = timed(lambda: ctx.nw_stats_banded(batch, sc, w), args.calls)
    else:
        sc = S.make_scoring(WB.NW_SPEC)
        batch, w = (NB.workload("b", args.scale)[0], 1024) if name == "w1024" else long_pairs(args.scale)
        got = ctx.nw_gaps_banded_wide(batch, sc, w)
        out["ran"] = {k: list(v) for k, v in ctx.last_call().items()}
        assert got[0].tobytes() == ctx.nw_score_banded_wide(batch, sc, w).tobytes(), "the score differs from nw_score_banded_wide's"
        out["gaps_call_ms"] = timed(lambda: ctx.nw_gaps_banded_wide(batch, sc, w), args.calls)
        out["stats_call_ms"] = timed(lambda: ctx.nw_stats_banded_wide(batch, sc, w), args.calls)
        if name == "w1024":
            def align_and_count():
                return host_runs(ctx.nw_align_banded_wide(batch, sc, w))

            ga, gb = align_and_count()
            assert np.array_equal(ga, got[1]) and np.array_equal(gb, got[2]), "the runs differ from nw_align_banded_wide's strings"
            out["align_count_call_ms"] = timed(align_and_count, max(2, args.calls // 5))
            out["aim2"] = "met" if out["gaps_call_ms"]["median"] < out["align_count_call_ms"]["median"] else "missed"
    out["pairs"] = batch.n_pairs
    out["gapopen_mean"] = round(float(np.mean(got[1].astype(np.int64) + got[2])), 3)
    ours = out.get("gaps_kernel_ms") or out["gaps_call_ms"]
    theirs = out.get("stats_kernel_ms") or out["stats_call_ms"]
    out["yardstick"] = "stats_kernel" if "stats_kernel_ms" in out else "stats_call"
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
        out = run_cross(ctx, args) if args.workload == "cross" else run(ctx, args.workload, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
