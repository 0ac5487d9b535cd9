"""Static VALU census of the check-lane check phases (decode_split.hip
spec_check_phase_lanes) in the headline kernel, by source line.

From a tools/census_isa.sh dump (compiled with line tables): every loop of the
kernel whose instructions come mostly from spec_check_phase_lanes, told apart
as the b2c-interval form (it has qkds::phi_bounds2's lines) or the psi-input
form, with its steps (tasks) counted from its transcendentals (a task of DC
entries: 3 DC per step in the psi-input form, 6 DC in the b2c-interval form),
then VALU instructions per step and per source line. The loop is unrolled over
two steps; where the compiler rotated it a one-step inner loop shows as well.

  python tools/check_lane_census.py file.s [--src qkd_ldpc_amd/csrc] [--dc 6]

--src: the sources the dump was compiled from (for the functions' line ranges).
"""
from __future__ import annotations

import collections
import os
import re
import sys

import isa_census as ic

TRANS = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32")


def func_range(path: str, name: str) -> tuple[int, int]:
    """Lines of the function whose definition line contains `name` (to the next line that is a lone '}')."""
    first = 0
    for n, line in enumerate(open(path), 1):
        if not first and name in line and not line.lstrip().startswith("//") and "(" in line and ";" not in line:
            first = n
        elif first and line.rstrip() == "}":
            return first, n
    raise SystemExit(f"{name} not found in {path}")


def main(argv):
    path = argv[1]
    src = argv[argv.index("--src") + 1] if "--src" in argv else os.path.join(os.path.dirname(__file__), "..",
                                                                             "qkd_ldpc_amd", "csrc")
    dc = int(argv[argv.index("--dc") + 1]) if "--dc" in argv else 6
    lo, hi = func_range(os.path.join(src, "decode_split.hip"), "void spec_check_phase_lanes(")
    b2lo, b2hi = func_range(os.path.join(src, "qkd_spec.h"), "void phi_bounds2(")
    name, lines = ic.kernel_lines(path, f"decode_split_kernelILi1ELi0ELi{dc}ELb1ELi1ELb0E")
    print(name)
    print(f"spec_check_phase_lanes: decode_split.hip:{lo}-{hi}; phi_bounds2: qkd_spec.h:{b2lo}-{b2hi}")
    pos = {l.split(":")[0]: i for i, l in enumerate(lines) if l.startswith(".LBB")}
    for i, l in enumerate(lines):
        t = l.split()
        if not (t and (t[0].startswith("s_cbranch") or t[0] == "s_branch") and t[-1] in pos and pos[t[-1]] < i):
            continue
        cur = ("?", 0)
        ops = collections.Counter()
        by = collections.Counter()
        byop = collections.defaultdict(collections.Counter)
        for x in lines[pos[t[-1]]:i + 1]:
            m = re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", x)
            if m:
                cur = (ic.FILES.get(m.group(1), m.group(1)), int(m.group(2)))
            elif x.startswith("\t") and not x.strip().startswith((";", ".")):
                o = ic.op(x)
                ops[o] += 1
                if o.startswith("v_"):
                    by[cur] += 1
                    byop[cur][o] += 1

        def count(*prefix):
            return sum(n for k, n in ops.items() if k.startswith(prefix))

        v, tr = count("v_"), count(*TRANS)
        own = sum(n for (f, ln), n in by.items() if f == "decode_split.hip" and lo <= ln <= hi)
        b2c = any(f == "qkd_spec.h" and b2lo <= ln <= b2hi for (f, ln) in by)
        per = (6 if b2c else 3) * dc
        # (the phase's own loops only: not the frame loop around them)
        if own < 50 or tr == 0 or tr % per or tr // per > 2:
            continue
        steps = tr // per
        print(f"\n== {'b2c-interval' if b2c else 'psi-input'} form, asm lines {pos[t[-1]]}..{i}, {steps} step(s) in the loop; "
              f"per step: VALU {v / steps:g} packed {count('v_pk_') / steps:g} transcendental {tr / steps:g} "
              f"v_cndmask {count('v_cndmask') / steps:g} v_cmp {count('v_cmp') / steps:g} "
              f"v_readlane/v_writelane {count('v_readlane', 'v_writelane') / steps:g} SALU {count('s_') / steps:g}")
        for (f, ln), n in sorted(by.items()):
            top = " ".join(f"{k[2:]}:{c / steps:g}" for k, c in byop[(f, ln)].most_common(4))
            print(f"   {f}:{ln:<5d} {n / steps:6g}  {top}")


if __name__ == "__main__":
    main(sys.argv)
