#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds kernel by kernel.

    python tools/compare_device_asm.py <build dir A> <build dir B> [name ...]

Reads <dir>/<name>-hip-amdgcn-amd-amdhsa-gfx950.s (what `hipcc -save-temps=obj` leaves beside the object) from both
directories (a name's file may be missing on one side) and compares, per kernel symbol over the UNION of the named
files -- a kernel that moved to another file compares against itself and is reported as moved -- the body (comments stripped, local labels renumbered in order of first
appearance, so instantiation order does not matter) and the kernel's metadata: register counts, private and group
segment sizes.  Prints one line per file of B, with
the register counts of every kernel that differs, and the verdict; exit status 1 on any difference.  A host-only refactor must
come out identical.
"""
import re
import sys
from pathlib import Path

NAMES = ["conv_igemm", "conv_bf16", "conv_mm16", "conv_wgrad", "map_head", "norm_ops", "norm_bf16"]
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(path):
    """{symbol: (normalised body lines, metadata dict)} of one assembly file."""
    lines = path.read_text().splitlines()
    meta, entry = {}, None
    start = lines.index("amdhsa.kernels:")
    for ln in lines[start + 1:]:                       # one YAML list entry per kernel, keys in alphabetical order
        if ln.startswith("  - "):
            entry = {}
        m = re.match(r"\s+(?:- )?(\.\w+):\s*(\S+)", ln)
        if entry is None or not m:
            continue
        if m.group(1) in META:
            entry[m.group(1)] = m.group(2)
        elif m.group(1) == ".symbol":
            meta[m.group(2)[:-len(".kd")]] = entry
    bodies, name, body = {}, None, []
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", ln):
            if name in meta:
                seen = {}
                text = "\n".join(body)
                for lab in LABEL.findall(text):
                    seen.setdefault(lab, ".L%d" % len(seen))
                bodies[name] = LABEL.sub(lambda mm: seen[mm.group(0)], text)
            name = None
            continue
        code = ln.split(";", 1)[0].rstrip()
        if code.strip():
            body.append(code)
    return {k: (bodies.get(k), meta[k]) for k in meta}


def side(d, names):
    """{symbol: (body, metadata, file name)} over the named files of one build directory."""
    out = {}
    for n in names:
        f = d / ("%s-hip-amdgcn-amd-amdhsa-gfx950.s" % n)
        if f.exists():
            out.update({k: v + (n,) for k, v in kernels(f).items()})
    return out


def regs(meta):
    return "vgpr %s sgpr %s agpr %s" % tuple(meta.get(k, "?") for k in META[:3])


def main():
    names = sys.argv[3:] or NAMES
    ka, kb = side(Path(sys.argv[1]), names), side(Path(sys.argv[2]), names)
    bad = 0
    only_a = sorted(set(ka) - set(kb))
    for n in names:
        mine = [k for k in kb if kb[k][2] == n]
        only_b = sorted(k for k in mine if k not in ka)
        both = [k for k in mine if k in ka]
        moved = [k for k in both if ka[k][2] != n]
        diff = [k for k in both if ka[k][0] != kb[k][0] or ka[k][1] != kb[k][1]]
        empty = [k for k in mine if kb[k][0] is None or len(kb[k][1]) != len(META)]
        print("%-11s kernels %3d  moved here %d  only in B %d  differ %d  unparsed %d"
              % (n, len(mine), len(moved), len(only_b), len(diff), len(empty)))
        for k in moved:
            print("     moved from %s: %s" % (ka[k][2], k))
        for k in only_b + empty:
            print("     only in B / unparsed:", k)
        for k in diff:
            print("     differs: %s\n         A: %s\n         B: %s" % (k, regs(ka[k][1]), regs(kb[k][1])))
        bad += len(only_b) + len(diff) + len(empty)
    for k in only_a:
        print("     only in A (%s): %s" % (ka[k][2], k))
    bad += len(only_a)
    print("verdict:", "IDENTICAL" if bad == 0 else "DIFFERENT (%d)" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
