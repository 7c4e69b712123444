#!/usr/bin/env python3
"""compare.py r17_*.jsonl ... -- parent against this tree, per workload line and per `*_ms` figure of the benchmark tools.

Each input line is a tool's JSON line with "tree" ("parent" | "this") and "run" in front (the job that wrote them ran the tool on
both trees in turn).  Per figure: the median of each tree's runs, the parent's own run-to-run range (max - min), and whether this
tree's median lies no further above the parent's median than that range.  Prints a markdown table; exit status 1 when a figure of a
call this change touches misses."""
import json
import statistics
import sys
from collections import defaultdict

# wall clock of calls whose host code this change does not touch: reported, not judged
UNTOUCHED = ("align_call_ms", "align_base_ms", "score_base_ms")

failed = 0
for path in sys.argv[1:]:
    runs = defaultdict(list)            # (tree, run) -> its lines in order
    for line in open(path):
        d = json.loads(line)
        runs[(d["tree"], d["run"])].append(d)
    figures = defaultdict(lambda: {"parent": [], "this": []})
    for (tree, run), lines in sorted(runs.items()):
        for k, d in enumerate(lines):
            tag = d["workload"] + (f" cols={d['band_strip_cols']}" if "band_strip_cols" in d else "") + (f" #{k}" if d["workload"] == "F" else "")
            for key, v in d.items():
                if key.endswith("_ms") and isinstance(v, (int, float)):
                    figures[(k, tag, key)][tree].append(v)
    print(f"\n### {path}\n\n| workload | figure | parent median | parent min .. max (range) | this median | this min .. max | above by | verdict |\n|---|---|---|---|---|---|---|---|")
    for (k, tag, key), v in sorted(figures.items()):
        p, t = v["parent"], v["this"]
        if not p or not t:
            continue
        pm, tm, rng = statistics.median(p), statistics.median(t), max(p) - min(p)
        judged = key not in UNTOUCHED and "kernel" not in key
        ok = tm - pm <= rng
        verdict = ("pass" if ok else "MISS") if judged else ("kernel: agrees" if ok else "kernel: differs") if "kernel" in key else "not judged"
        failed += judged and not ok
        print(f"| {tag} | `{key}` | {pm:.4g} | {min(p):.4g} .. {max(p):.4g} ({rng:.3g}) | {tm:.4g} | {min(t):.4g} .. {max(t):.4g} | {tm - pm:+.3g} | {verdict} |")
sys.exit(1 if failed else 0)
