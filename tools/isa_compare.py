#!/usr/bin/env python3
"""Compare two device-assembly files of one HIP source, function by function.

  hipcc <csrc/Makefile's FLAGS> --cuda-device-only -S file.hip -o before.s   (at one commit)
  hipcc <csrc/Makefile's FLAGS> --cuda-device-only -S file.hip -o after.s    (at another)
  python tools/isa_compare.py before.s after.s [--rename OLD=NEW ...]

Each file is split at its `.type NAME,@function` ... `.Lfunc_end` pairs.  Comments,
directives and blank lines are dropped, and local labels (.LBB3_17, .Ltmp5, .Lpost_getpc2,
...) are renumbered in order of first appearance, so a function that only moved within
the file compares equal.  --rename substitutes NEW for the regular expression OLD in the
first file's text (a mangled name, or a piece of one, that changed between the two), e.g.
--rename '(kConv1LPILi.ELi.ELi.E)Lb0E=\\1' for a dropped template argument.
One line per function:
  same NAME LINES | DIFF NAME LINES_BEFORE LINES_AFTER DIFFERING | NEW NAME LINES | GONE NAME LINES
Exit status 1 when any function differs.
"""
import argparse
import collections
import re
import sys

TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
END = re.compile(r"^\.Lfunc_end\d+:")
LOCAL = re.compile(r"\.L[A-Za-z_$]+\d+(?:_\d+)?")


def functions(path, renames):
    text = open(path).read()
    for old, new in renames:
        text = re.sub(old, new, text)
    out, name, body = {}, None, []
    for line in text.split("\n"):
        m = TYPE.match(line)
        if m:
            name, body = m.group(1), []
        elif name and END.match(line):
            out[name] = normalise(body)
            name = None
        elif name:
            body.append(line)
    return out


def normalise(body):
    seen, lines = {}, []
    for line in body:
        line = line.split(";", 1)[0].strip()
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue  # comment, blank or directive (labels stay)
        lines.append(LOCAL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), line))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    fa = functions(a.before, [r.split("=", 1) for r in a.rename])
    fb = functions(a.after, [])
    differ = False
    for name in sorted(set(fa) | set(fb)):
        if name not in fa:
            print("NEW", name, len(fb[name]))
        elif name not in fb:
            print("GONE", name, len(fa[name]))
        elif fa[name] == fb[name]:
            print("same", name, len(fa[name]))
        else:
            # lines of one side without a partner on the other (0: the same lines in another order)
            ca, cb = collections.Counter(fa[name]), collections.Counter(fb[name])
            n = max(sum((ca - cb).values()), sum((cb - ca).values()))
            print("DIFF", name, len(fa[name]), len(fb[name]), n)
            differ = True
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
