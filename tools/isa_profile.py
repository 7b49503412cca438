#!/usr/bin/env python3
"""Compare the gfx950 kernels of two assembly files, symbol by symbol (the gate of a refactor that must not change device code).
    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -cuid=cmp --cuda-device-only -S file.hip -o file.s     (parent and head)
    python tools/isa_profile.py parent/file.s head/file.s
Per kernel symbol found in both files, one verdict:
  identical       the instruction lines (comments and directives dropped, `.LBB<n>_` renumbered) and the `.amdhsa_` block are equal
  profile-equal   the `.amdhsa_` block, the register / spill / LDS figures of the metadata and the per-mnemonic counts of every
                  matrix, memory, LDS, transcendental, wait, barrier and branch instruction are equal; the mnemonics whose
                  counts differ (address arithmetic, moves, nops) and the SGPR spill counts are listed
  different       anything else; the exit status is then 1
Symbols that only one file has are listed and not judged (a file split moves them: compare the other file too).
"""
import collections
import re
import sys
HEAVY = ("v_mfma", "buffer_", "global_", "flat_", "scratch_", "ds_", "v_exp", "v_rcp", "v_log", "v_rsq", "v_sqrt", "s_waitcnt",
         "s_barrier", "s_sleep", "s_getreg", "s_memrealtime", "s_and_saveexec", "s_or_saveexec", "s_cbranch")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    """symbol -> (instruction lines, .amdhsa_ lines, metadata figures)"""
    text = open(path).read().split("\n")
    hsa, cur = {}, None
    for ln in text:
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):
            cur = hsa.setdefault(s.split()[1], [])
        elif s == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and s.startswith(".amdhsa_"):
            cur.append(s)
    meta, fig = {}, {}
    for ln in text:                         # amdhsa.kernels: one list item per kernel at indent 2, its keys at indent 4
        m = re.match(r"  [- ] (\.\w+):\s*(\S+)\s*$", ln)
        fig = {} if ln.startswith("  - ") else fig
        if m and m.group(1) == ".name":
            meta[m.group(2)] = fig
        elif m:
            fig[m.group(1)] = m.group(2)
    out = {}
    for sym in hsa:                         # the symbol's instruction lines and labels, up to .Lfunc_end
        body, on = [], False
        for ln in text:
            if ln.startswith(sym + ":"):
                on = True
            elif on and ln.startswith(".Lfunc_end"):
                break
            elif on:
                s = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip())
                if s and (not s.startswith(".") or s.endswith(":")):
                    body.append(s)
        out[sym] = (body, hsa[sym], meta.get(sym, {}))
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    worst = 0
    for sym in sorted(set(ka) ^ set(kb)):
        print(f"only in {a if sym in ka else b}: {sym}")
    for sym in sorted(set(ka) & set(kb)):
        (ia, ha, ma), (ib, hb, mb) = ka[sym], kb[sym]
        if ia == ib and ha == hb:
            print(f"identical       {sym}  ({len(ia)} lines)")
            continue
        ca, cb = (collections.Counter(s.split()[0] for s in i if not s.endswith(":")) for i in (ia, ib))
        diff = sorted(m for m in set(ca) | set(cb) if ca[m] != cb[m])
        heavy = [m for m in diff if m.startswith(HEAVY)]
        figs = [k for k in META if ma.get(k) != mb.get(k)]
        ok = ha == hb and not heavy and not figs
        worst |= not ok
        print(f"{'profile-equal' if ok else 'different':<16}{sym}  ({len(ia)} -> {len(ib)} lines; SGPR spills "
              f"{ma.get('.sgpr_spill_count')} -> {mb.get('.sgpr_spill_count')})")
        if ha != hb:
            print("    .amdhsa_ block: " + "; ".join(f"{x} -> {y}" for x, y in zip(ha, hb) if x != y))
        for k in figs:
            print(f"    {k}: {ma.get(k)} -> {mb.get(k)}")
        for m in diff:
            print(f"    {'HEAVY ' if m in heavy else ''}{m}: {ca[m]} -> {cb[m]}")
    return int(worst or not set(ka) & set(kb))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]) if len(sys.argv) == 3 else __doc__)
