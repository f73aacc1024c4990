#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files (hipcc --offload-arch=gfx950 --cuda-device-only -S) of the same source
before and after a change that must not move the instruction stream.

    tools/isa_compare.py OLD.s NEW.s [--rename REGEX REPLACEMENT] [--only PREFIX ...]

Per kernel of OLD (after --rename has been applied to every symbol in it): the instructions between its label and its end
marker with comments and label numbers dropped, and vgpr / agpr / sgpr counts, LDS, scratch and kernarg bytes from the code
object metadata.  One line per kernel; the exit status is 1 when a kernel differs or the two lists of kernels differ."""
import argparse
import difflib
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def kernels(text):
    """name -> (normalised body lines, metadata tuple)"""
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        get = lambda key: re.search(r"^\s*" + re.escape(key) + r":\s*(\S+)", block, re.M).group(1)
        meta[get(".name")] = tuple(int(get(k)) for k in META)
    out = {}
    for name in meta:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S)
        body = []
        for line in m.group(1).split("\n"):
            line = line.split(";")[0].rstrip()
            if line:
                body.append(re.sub(r"\.L(BB|func_end|Ltmp)\d+", r".L\1", line))
        out[name] = (body, meta[name])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    ap.add_argument("--only", nargs="*", default=[], help="kernel-name substrings to report (default: all)")
    a = ap.parse_args()
    old_text = open(a.old).read()
    names_before = set(kernels(old_text))
    renamed = old_text
    for rx, repl in a.rename:
        renamed = re.sub(rx, repl, renamed)
    old, new = kernels(renamed), kernels(open(a.new).read())
    back = {}
    for n in names_before:
        m = n
        for rx, repl in a.rename:
            m = re.sub(rx, repl, m)
        back[m] = n
    bad = 0
    for name in sorted(set(old) | set(new)):
        if a.only and not any(s in name for s in a.only):
            continue
        if name not in old or name not in new:
            print(f"{back.get(name, '-') if name in old else '-'} {name if name in new else '-'} ONLY IN {'OLD' if name in old else 'NEW'}")
            bad += 1
            continue
        (ob, om), (nb, nm) = old[name], new[name]
        v, ag, s, lds, scr, ka = nm
        regs = f"vgpr {v} agpr {ag} sgpr {s} lds {lds} scratch {scr} kernarg {ka} insts {len(nb)}"
        if ob == nb and om == nm:
            verdict = "identical"
        else:
            d = sum(1 for l in difflib.unified_diff(ob, nb, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            verdict = f"DIFFERENT: {d} lines" + (f", metadata {om} -> {nm}" if om != nm else "")
            bad += 1
        print(f"{back[name]} {name} {regs} {verdict}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
