#!/usr/bin/env python3
"""Kernel-by-kernel ISA comparison of two csrc trees (a refactor must leave the machine code of the kernels it does not mean to change alone).

  python scripts/isa_diff.py <parent csrc dir> <changed csrc dir> [file.hip ...]      default: every *.hip of either tree
  ISA_DIFF_SHOW=<text>   also print a unified diff of the instruction streams of the DIFF kernels whose name contains <text>

Both sides are compiled with isa_audit.compile_to_isa (the Makefile's flags).  Per kernel: demangled name (without its parameter list), SAME / DIFF / NEW / GONE,
and instruction count, VGPRs and scratch bytes of the parent -> the change.  Two kernels are SAME when their instruction streams are equal
after comments, labels and assembler directives are dropped (branch targets are compared by their number within the function).
A kernel missing from the same-named file is looked up by name in the other files of that tree: a kernel that only moved prints
SAME with both file names.  The lookup goes by the demangled name alone (kernels sit in anonymous namespaces) and takes the first file that has it:
a new kernel that shares its name with one elsewhere in the tree is compared with that one, not listed as NEW.  Exit code 1 when any kernel is not SAME.
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
    both = lambda pat: sorted({os.path.basename(f) for d in (pdir, cdir) for f in glob.glob(os.path.join(d, pat))})
    files = [os.path.basename(f) for f in sys.argv[3:]] or both("*.hip")
    jobs = [os.path.join(d, f) for f in files for d in (pdir, cdir) if os.path.exists(os.path.join(d, f))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        texts = dict(zip(jobs, ex.map(compile_to_isa, jobs)))
    old, new = ({f: kernels(texts.get(os.path.join(d, f), "")) for f in files} for d in (pdir, cdir))
    where = lambda side, k: next((f for f in files if k in side[f]), None)      # a kernel that moved: looked up by name in the whole tree
    ndiff = total = 0
    for f in files:
        for k in sorted(set(old[f]) | set(new[f])):
            fo, fn = (f if k in old[f] else where(old, k)), (f if k in new[f] else where(new, k))
            if k not in new[f] and fn:
                continue                                                        # listed under the file that has it now
            o, n = old[fo][k] if fo else None, new[fn][k] if fn else None
            tag = "GONE" if n is None else "NEW " if o is None else "SAME" if o[0] == n[0] else "DIFF"
            fmt = lambda s: "     -     -    -" if s is None else f"{len(s[0]):6d} {s[1]:5d} {s[2]:4d}"
            name = f if fo in (None, f) else f"{fo} -> {f}"
            print(f"{name:16s} {tag}  instr/vgpr/scratch {fmt(o)}  -> {fmt(n)}  {k.split('(')[0]}")
            show = os.environ.get("ISA_DIFF_SHOW")
            if tag == "DIFF" and show and show in k:
                print("\n".join(difflib.unified_diff(o[0], n[0], "parent", "change", n=2, lineterm="")))
            total += 1
            ndiff += tag != "SAME"
    print(f"{total} kernels, {ndiff} not SAME")
    return 1 if ndiff else 0


if __name__ == "__main__":
    sys.exit(main())
