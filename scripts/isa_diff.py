#!/usr/bin/env python3
"""Kernel-by-kernel ISA comparison of two csrc trees (a refactor must leave the machine code of the kernels it does not mean to change alone).

  python scripts/isa_diff.py <parent csrc dir> <changed csrc dir> [file.hip ...]      default: every *.hip of the changed tree
  ISA_DIFF_SHOW=<text>   also print a unified diff of the instruction streams of the DIFF kernels whose name contains <text>

Both sides are compiled with isa_audit.compile_to_isa (the Makefile's flags).  Per kernel: demangled name (without its parameter list), SAME / DIFF / NEW / GONE,
and instruction count, VGPRs and scratch bytes of the parent -> the change.  Two kernels are SAME when their instruction streams are equal
after comments, labels and assembler directives are dropped (branch targets are compared by their number within the function).
Exit code 1 when any kernel is not SAME.
"""
import concurrent.futures
import difflib
import glob
import os
import re
import sys

from isa_audit import compile_to_isa, demangle


def kernels(txt):
    """demangled name -> (instruction list, vgprs, scratch)"""
    meta = {}
    for m in re.finditer(r"\.name:\s+(_Z\S+)\n((?:\s+\.\w+:.*\n)+)", txt):
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2))
        vg = re.search(r"\.vgpr_count:\s+(\d+)", m.group(2))
        if ps:
            meta[m.group(1)] = (int(vg.group(1)) if vg else -1, int(ps.group(1)))
    body, name = {}, None
    for ln in txt.split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m and m.group(1) in meta:
            name = m.group(1); body[name] = []
            continue
        if name is None:
            continue
        t = ln.split(";")[0].strip()
        if t.startswith(".Lfunc_end") or t.startswith(".size"):      # not the first s_endpgm: a kernel with an early return has several
            name = None
        elif t and not t.startswith(".") and not t.endswith(":"):
            body[name].append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
    names = list(body)
    return {d: (body[n],) + meta[n] for n, d in zip(names, demangle(names))} if names else {}


def main():
    if len(sys.argv) < 3:
        print(__doc__); return 2
    pdir, cdir = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    files = [os.path.basename(f) for f in sys.argv[3:]] or sorted(os.path.basename(f) for f in glob.glob(os.path.join(cdir, "*.hip")))
    jobs = [os.path.join(d, f) for f in files for d in (pdir, cdir)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        texts = list(ex.map(compile_to_isa, jobs))
    ndiff = total = 0
    for i, f in enumerate(files):
        old, new = kernels(texts[2 * i]), kernels(texts[2 * i + 1])
        for k in sorted(set(old) | set(new)):
            o, n = old.get(k), new.get(k)
            tag = "GONE" if n is None else "NEW " if o is None else "SAME" if o[0] == n[0] else "DIFF"
            fmt = lambda s: "     -     -    -" if s is None else f"{len(s[0]):6d} {s[1]:5d} {s[2]:4d}"
            print(f"{f:16s} {tag}  instr/vgpr/scratch {fmt(o)}  -> {fmt(n)}  {k.split('(')[0]}")
            show = os.environ.get("ISA_DIFF_SHOW")
            if tag == "DIFF" and show and show in k:
                print("\n".join(difflib.unified_diff(o[0], n[0], "parent", "change", n=2, lineterm="")))
            total += 1
            ndiff += tag != "SAME"
    print(f"{total} kernels, {ndiff} not SAME")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
