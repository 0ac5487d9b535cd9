#!/usr/bin/env python3
"""Compare two directories of device assembly kernel by kernel (CPU only).

    python tools/kernel_isa_diff.py PARENT_DIR NEW_DIR

Each directory holds the .s files of one tree's .hip files, compiled with the
Makefile's own CXXFLAGS and FILE_FLAGS plus `--cuda-device-only -S`. A move of
kernels between files must leave every kernel's instructions and descriptor as
they were: the functions (`_Z...:` or a C name, to `.Lfunc_endN:`) and the
`.amdhsa_kernel NAME ... .end_amdhsa_kernel` blocks of all files of a side are
keyed by symbol, comments stripped and the per-function counters of local
labels rewritten, and compared as text. Exit status 0: the same kernels, each
defined once, no difference."""
import difflib
import glob
import os
import re
import sys

LOCAL = [(re.compile(r"\.LBB\d+_(\d+)"), r".LBB_\1"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"),
         (re.compile(r"\.Ltmp\d+"), ".Ltmp")]


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    for rx, to in LOCAL:
        line = rx.sub(to, line)
    return line


def parse(text, funcs, descs, seen):
    """Adds text's functions and kernel descriptors (symbol -> lines) to funcs / descs."""
    func = desc = None
    for raw in text.splitlines():
        line = clean(raw)
        if not line.strip():
            continue
        m = re.match(r"([A-Za-z_][\w$.]*):$", line)
        if m and not m.group(1).startswith(".L"):
            func = funcs[m.group(1)] = []
            seen.append(m.group(1))
        elif line.strip().startswith(".amdhsa_kernel "):
            desc = descs.setdefault(line.split()[1], [])
        elif desc is not None:             # (the descriptor sits inside its function's text)
            desc.append(line)
            if ".end_amdhsa_kernel" in line:
                desc = None
        elif func is not None:
            func.append(line)
            if re.match(r"\.Lfunc_end:?$", line):
                func = None


def parse_dir(path):
    funcs, descs, seen = {}, {}, []
    for f in sorted(glob.glob(os.path.join(path, "*.s"))):
        parse(open(f).read(), funcs, descs, seen)
    # (kernels are the symbols with a descriptor; other labels are data)
    return {k: v for k, v in funcs.items() if k in descs}, descs, {k for k in descs if seen.count(k) > 1}


def compare(a, b, out=sys.stdout):
    (fa, da, dupa), (fb, db, dupb) = a, b
    only_a, only_b = sorted(set(da) - set(db)), sorted(set(db) - set(da))
    both = sorted(set(da) & set(db))
    isa = [k for k in both if fa.get(k) != fb.get(k)]
    desc = [k for k in both if da[k] != db[k]]
    dups = sorted(dupa | dupb)
    print(f"kernels: parent {len(da)}, change {len(db)}, compared {len(both)}", file=out)
    print(f"instruction lines compared: {sum(len(fa.get(k, ())) for k in both)}", file=out)
    for title, names in (("only in the parent", only_a), ("only in the change", only_b),
                         ("defined more than once", dups), ("instructions differ", isa), ("descriptor differs", desc)):
        print(f"{title}: {len(names)}", file=out)
        for k in names:
            print(f"  {k}", file=out)
            if names is isa:
                d = difflib.unified_diff(fa.get(k, []), fb.get(k, []), "parent", "change", lineterm="", n=1)
                for line in list(d)[:12]:
                    print(f"    {line}", file=out)
    return 1 if only_a or only_b or dups or isa or desc else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(compare(parse_dir(sys.argv[1]), parse_dir(sys.argv[2])))
