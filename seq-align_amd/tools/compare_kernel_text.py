#!/usr/bin/env python3
"""compare_kernel_text.py OLD.s NEW.s [--rename OLD_KERNEL=NEW_KERNEL ...] [--show]

Did a refactor change a kernel's instructions?  Takes two device assembly files (hipcc --cuda-device-only -S with the
Makefile's flags, one of the parent and one of the tree) and prints per kernel "same" or "differs by N lines".

It is a plain text compare and inspects nothing else.  Per kernel the text from its label to its end label -- the
instructions and the .amdhsa_ descriptor -- with comments dropped, blanks squeezed, local labels renumbered per function
(.LBB7_3 -> .LBB_3) and every mangled name replaced by one word.  Kernels are paired by their template's name and its
literal arguments (Li.. / Lb.. of the mangled name, in order), so a kernel may move to another namespace, get another
parameter type or gain a class argument; --rename pairs a template that got a new name.  A kernel that only one file holds
is reported.  Exit status 1 when anything differs or is missing.
"""
import argparse
import difflib
import re
import sys

LABEL = re.compile(r"^(_Z\w+):")
END = re.compile(r"^\.Lfunc_end\d+:")


def kernel_key(mangled):
    """(template name, literal template arguments) of a mangled kernel name"""
    s = mangled[2:]
    if s.startswith("N"):
        s = s[1:]
    name = None
    while True:
        m = re.match(r"(\d+)", s)
        if not m:
            break
        n = int(m.group(1))
        name = s[m.end():m.end() + n]
        s = s[m.end() + n:]
    args_end = s.find("EEv")
    args = s if args_end < 0 else s[:args_end + 1]
    return name, tuple(re.findall(r"L[ib]n?\d+E", args))


def normal(line):
    line = line.split(";", 1)[0]
    line = re.sub(r"\.L(BB|tmp|func_end|func_begin)\d+(_\d+)?", lambda m: ".L%s%s" % (m.group(1), m.group(2) or ""), line)
    line = re.sub(r"\b_Z\w+", "SYM", line)
    return " ".join(line.split())


def kernels(path, rename):
    out, cur, body = {}, None, None
    with open(path) as f:
        for line in f:
            m = LABEL.match(line)
            if m and cur is None:
                cur, body = m.group(1), []
                continue
            if cur is None:
                continue
            if END.match(line):
                name, args = kernel_key(cur)
                key = (rename.get(name, name), args)
                if key in out:
                    sys.exit("%s: two kernels read as %s%s: pair them by hand" % (path, key[0], list(key[1])))
                out[key] = [t for t in (normal(x) for x in body) if t]
                cur = None
                continue
            body.append(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="OLD.s's template OLD is NEW.s's NEW")
    ap.add_argument("--only", metavar="REGEX", help="kernels of NEW.s (and renamed ones of OLD.s) whose template name matches")
    ap.add_argument("--show", action="store_true", help="print the differing lines")
    a = ap.parse_args()
    rename = dict(r.split("=", 1) for r in a.rename)
    old, new = kernels(a.old, rename), kernels(a.new, {})
    if a.only:
        old = {k: v for k, v in old.items() if re.search(a.only, k[0])}
        new = {k: v for k, v in new.items() if re.search(a.only, k[0])}
    same = bad = 0
    for key in sorted(set(old) | set(new)):
        label = "%s<%s>" % (key[0], ", ".join(x[1:-1] for x in key[1]))
        if key not in old or key not in new:
            print("%-60s only in %s" % (label, a.new if key in new else a.old))
            bad += 1
            continue
        if old[key] == new[key]:
            print("%-60s same (%d lines)" % (label, len(new[key])))
            same += 1
            continue
        ops = [o for o in difflib.SequenceMatcher(None, old[key], new[key], autojunk=False).get_opcodes() if o[0] != "equal"]
        n = sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops)
        print("%-60s differs by %d lines (of %d)" % (label, n, len(new[key])))
        bad += 1
        if a.show:
            for _, i1, i2, j1, j2 in ops:
                for x in old[key][i1:i2]:
                    print("    - " + x)
                for x in new[key][j1:j2]:
                    print("    + " + x)
    print("%d kernels: %d same, %d not" % (same + bad, same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
