#!/usr/bin/env python3
"""Static instruction counts of the 4 x 32 tile kernels (csrc/gdmlp_x6.hip, csrc/ss2d_front_x6.hip), per kernel and per section.

  python scripts/tile_diet_isa.py [label]      cross-compiles for gfx950 with the Makefile's flags (scripts/isa_audit.py) and prints one
                                               table; no GPU is needed.  profiles/tile_diet_isa.txt holds its output for two commits.

Sections: the chunk loop (gdMlp / vss_back: `for j < NCH`) is the span of the overlapping backward-branch regions around the one with
the most barriers; what stands in front of it is the prologue, what follows the epilogue.  A kernel without such a loop (the SS2D front) is one section.  Counts are static and per
wave: an instruction inside a branch counts once whether or not the branch is taken.  Classes only:
  VALU      v_* except the MFMAs          MFMA     v_mfma*             LDS      ds_*
  cnd       v_cndmask*                    a64      v_lshl_add_u64, v_mad_i64_i32, v_mad_u64_u32 (64-bit per-lane address arithmetic)
  exbr      s_cbranch_exec*               div      v_div_scale*        vmem     global_load* / global_store*
"""
import importlib.util
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(HERE, "isa_audit.py"))
ia = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ia)

FILES = ("gdmlp_x6.hip", "ss2d_front_x6.hip")
KERNELS = re.compile(r"^(gdmlp_x6_kernel<(3, 2, 2|5, 3, 1), false>|vss_back_x6_kernel<3, 2, 2>|ss2d_front_x6_kernel<3, 4[08]>)")
CLASSES = (("VALU", lambda m: m.startswith("v_") and not m.startswith("v_mfma")), ("MFMA", lambda m: m.startswith("v_mfma")),
           ("LDS", lambda m: m.startswith("ds_")), ("cnd", lambda m: m.startswith("v_cndmask")),
           ("a64", lambda m: m.startswith(("v_lshl_add_u64", "v_mad_i64_i32", "v_mad_u64_u32"))),
           ("exbr", lambda m: m.startswith("s_cbranch_exec")), ("div", lambda m: m.startswith("v_div_scale")),
           ("vmem", lambda m: m.startswith(("global_load", "global_store"))))


def kernels_of(txt):
    """[(mangled name, vgprs, scratch, [(label | None, mnemonic, operands)])]"""
    meta = {}
    for m in re.finditer(r"\.name:\s+(_Z\S+)\n((?:\s+\.\w+:.*\n)+)", txt):
        ps, vg = re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2)), re.search(r"\.vgpr_count:\s+(\d+)", m.group(2))
        if ps:
            meta[m.group(1)] = (int(vg.group(1)) if vg else -1, int(ps.group(1)))
    out, name = {}, None
    for ln in txt.split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m and m.group(1) in meta:
            name = m.group(1)
            out[name] = []
            continue
        if name is None:
            continue
        t = ln.split(";")[0].strip()
        lab = re.match(r"^(\.LBB\d+_\d+):", t)
        if lab:
            out[name].append((lab.group(1), None, ""))
        elif t and not t.startswith("."):
            parts = t.split(None, 1)
            out[name].append((None, parts[0], parts[1] if len(parts) > 1 else ""))
            if parts[0] == "s_endpgm":
                name = None
    return [(k, meta[k][0], meta[k][1], v) for k, v in out.items()]


def sections(items):
    """-> [(section name, [mnemonics])]: prologue / chunk loop / epilogue, or the whole kernel where no loop holds MFMAs"""
    at = {lab: i for i, (lab, _, _) in enumerate(items) if lab}
    loops = []
    for i, (_, mn, ops) in enumerate(items):
        if mn and mn.startswith(("s_cbranch", "s_branch")) and ops.strip() in at and at[ops.strip()] < i:
            lo = at[ops.strip()]
            loops.append((sum(1 for _, m, _ in items[lo:i] if m == "s_barrier"),
                          sum(1 for _, m, _ in items[lo:i] if m and m.startswith("v_mfma")), lo, i + 1))
    ins = lambda part: [m for _, m, _ in part if m]
    if not any(l[1] for l in loops):
        return [("whole", ins(items))]
    # the compiler lays a loop with wave-uniform branches out as several overlapping backward-branch regions: start from the one with
    # the most barriers (the chunk loop has two) and MFMAs and take in every region that overlaps the span
    _, _, lo, hi = max(loops)
    grown = True
    while grown:
        grown = False
        for _, _, a, b in loops:
            if a < hi and b > lo and (a < lo or b > hi):
                lo, hi, grown = min(lo, a), max(hi, b), True
    return [("prologue", ins(items[:lo])), ("chunk loop", ins(items[lo:hi])), ("epilogue", ins(items[hi:])), ("whole", ins(items))]


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "working tree"
    print(f"== {label}")
    print(f"{'kernel':36s} {'section':10s} " + " ".join(f"{c:>5s}" for c, _ in CLASSES) + "  instr")
    for f in FILES:
        ks = kernels_of(ia.compile_to_isa(os.path.join(ia.CSRC, f)))
        for (mangled, vg, sc, items), name in zip(ks, ia.demangle([k[0] for k in ks])):
            name = name.split("(")[0]
            if not KERNELS.match(name):
                continue
            for sec, mns in sections(items):
                print(f"{name:36s} {sec:10s} " + " ".join(f"{sum(1 for m in mns if is_(m)):5d}" for _, is_ in CLASSES) + f" {len(mns):6d}")
            print(f"{name:36s} {'registers':10s} vgpr {vg}, scratch {sc} B")
    return 0


if __name__ == "__main__":
    sys.exit(main())
