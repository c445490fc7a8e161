#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds kernel by kernel.

    python tools/compare_device_asm.py <build dir A> <build dir B> [name ...]

Reads <dir>/<name>-hip-amdgcn-amd-amdhsa-gfx950.s (what `hipcc -save-temps=obj` leaves beside the object) from both
directories and compares, per kernel symbol, the body (comments stripped, local labels renumbered in order of first
appearance, so instantiation order does not matter) and the kernel's metadata: register counts, private and group
segment sizes.  Prints one line per file and the verdict; exit status 1 on any difference.  A host-only refactor must
come out identical.
"""
import re
import sys
from pathlib import Path

NAMES = ["conv_igemm", "conv_bf16", "conv_mm16", "conv_wgrad", "map_head"]
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


def main():
    a, b = Path(sys.argv[1]), Path(sys.argv[2])
    bad = 0
    for n in sys.argv[3:] or NAMES:
        f = "%s-hip-amdgcn-amd-amdhsa-gfx950.s" % n
        ka, kb = kernels(a / f), kernels(b / f)
        only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        body = [k for k in ka if k in kb and ka[k][0] != kb[k][0]]
        meta = [k for k in ka if k in kb and ka[k][1] != kb[k][1]]
        empty = [k for k in ka if ka[k][0] is None or len(ka[k][1]) != len(META)]
        print("%-11s kernels %3d / %3d  only in A %d  only in B %d  bodies differ %d  metadata differs %d  unparsed %d"
              % (n, len(ka), len(kb), len(only_a), len(only_b), len(body), len(meta), len(empty)))
        for k in only_a + only_b + body + meta + empty:
            print("    ", k)
        bad += len(only_a) + len(only_b) + len(body) + len(meta) + len(empty)
    print("verdict:", "IDENTICAL" if bad == 0 else "DIFFERENT (%d)" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
