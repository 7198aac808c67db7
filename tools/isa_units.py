"""Two builds of the library, translation unit by translation unit (no device needed):
  python tools/isa_units.py <parent.so> <tree.so> [substring of the kernels whose units are new, default k_dist; - for none]
                            [substrings of kernels that are expected to differ ...]
tools/isa_diff.py keys every kernel by its symbol; a kernel defined inline in a header is emitted by every unit that uses it, and
with a unit added the copy that wins the key is another one.  Here the code objects are paired in link order, the tree's new units
(those that hold a kernel with the given substring) set aside, and every pre-existing symbol compared with its own unit's copy:
identical, differing in pc-relative address operands only, or differing otherwise (exit status 1).  A kernel named as expected to
differ is counted on its own and does not fail the run."""
import sys, re, subprocess, os, tempfile, difflib
LLVM = "/opt/rocm/lib/llvm/bin"
def units(lib):
    out = []
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "lib.so"); os.symlink(os.path.abspath(lib), so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], cwd=d, capture_output=True)
        def key(f):
            m = re.findall(r"\d+", f); return [int(x) for x in m]
        for co in sorted((f for f in os.listdir(d) if "gfx950" in f), key=key):
            asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", os.path.join(d, co)], capture_output=True, text=True).stdout
            ks = {}
            for f in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", asm):
                m = re.match(r"[0-9a-f]+ <([^>]+)>:", f)
                if m:
                    code = [re.sub(r"\s*//.*", "", ln).strip() for ln in f.splitlines()[1:] if ln.startswith("\t")]
                    ks[m.group(1)] = [c for c in code if c and c != "..." and not c.startswith("s_nop") and not c.startswith("s_code_end")]      # (padding behind a unit's last kernel)
            out.append((co, ks))
    return out
a, b = units(sys.argv[1]), units(sys.argv[2])
NEW = sys.argv[3] if len(sys.argv) > 3 else "k_dist"
MAY = sys.argv[4:]
new = [(co, ks) for co, ks in b if NEW != "-" and any(NEW in n and NEW + "_" not in n for n in ks)]
b = [(co, ks) for co, ks in b if (co, ks) not in new]
print(f"parent: {len(a)} code objects; tree: {len(b)} + {len(new)} new (the units of {NEW})")
assert len(a) == len(b)
tot = same = addr = other = 0
may = {}
for (ca, ka), (cb, kb) in zip(a, b):
    only_b = sorted(set(kb) - set(ka)); only_a = sorted(set(ka) - set(kb))
    if only_a or only_b: print(f"  unit {ca}: only in parent {only_a}; only in tree {only_b}")
    for n in sorted(set(ka) & set(kb)):
        tot += 1
        if ka[n] == kb[n]: same += 1; continue
        d = [(x, y) for x, y in zip(ka[n], kb[n]) if x != y]
        pcrel = len(ka[n]) == len(kb[n]) and all(re.sub(r"0x[0-9a-f]+|\b\d+\b", "#", x) == re.sub(r"0x[0-9a-f]+|\b\d+\b", "#", y) and x.split()[0] in ("s_add_u32", "s_addc_u32", "s_getpc_b64", "s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz", "s_cbranch_execnz") for x, y in d)
        if pcrel: addr += 1
        elif any(m in n and m + "_" not in n for m in MAY):      # (k_dist, not k_dist_draw: the guard of the new-unit selection)
            k = next(m for m in MAY if m in n and m + "_" not in n); may[k] = may.get(k, 0) + 1
        else:
            other += 1; print(f"  DIFFERS unit {ca}: {n}: {len(ka[n])} -> {len(kb[n])} instructions, {len(d)} lines")
        if pcrel and addr <= 3: print(f"  pc-relative only, e.g. {n[:60]}: {d[0][0]}  ->  {d[0][1]}")
print(f"{tot} pre-existing kernel symbols compared unit by unit: {same} identical, {addr} differ in pc-relative address operands only, {other} differ otherwise"
      + "".join(f", {v} of {k} differ as expected" for k, v in sorted(may.items())))
for co, ks in new:
    print(f"  new unit {co}: " + ", ".join(sorted(n for n in ks if NEW in n))[:400])
sys.exit(1 if other else 0)
