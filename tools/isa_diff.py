"""Two builds of the library, kernel by kernel: disassembly and code-object notes (no device needed).
  python tools/isa_diff.py <parent.so> <tree.so>
Prints one line per kernel that differs - regs = (VGPRs, spilled VGPRs, SGPRs, scratch bytes, LDS bytes, kernarg bytes), occupancy in
waves per SIMD from the VGPR count (512 registers, granule 8, at most 8 waves), instruction counts, differing lines - then a census.
A line starts with FAIL if the kernel's spills / scratch / LDS / kernarg differ or its occupancy falls, with RISE if its occupancy
rises (fewer registers).  Exit status 1 if the symbol sets differ or any line is a FAIL; rises are counted in the last line."""
import difflib, os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(lib):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "lib.so")
        os.symlink(os.path.abspath(lib), so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], cwd=d, capture_output=True)
        for co in sorted(f for f in os.listdir(d) if "gfx950" in f):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", os.path.join(d, co)], capture_output=True, text=True).stdout
            regs = {}
            for b in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                g = lambda k: (re.search(rf"\.{k}:\s+(\S+)", b) or [None, "0"])[1]
                regs[g("name")] = tuple(int(g(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "private_segment_fixed_size",
                                                           "group_segment_fixed_size", "kernarg_segment_size"))
            asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", os.path.join(d, co)], capture_output=True, text=True).stdout
            for f in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", asm):
                m = re.match(r"[0-9a-f]+ <([^>]+)>:", f)
                if m and m.group(1) in regs:
                    # mnemonic and operands only: no addresses, no encodings
                    code = [re.sub(r"\s*//.*", "", ln).strip() for ln in f.splitlines()[1:] if ln.startswith("\t")]
                    out[m.group(1)] = (regs[m.group(1)], [c for c in code if c and not c.startswith("s_nop") and not c.startswith("s_code_end")])
    return out


def occupancy(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
names = sorted(set(a) | set(b))
dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()))
bad = rises = 0
census = {}
for n in names:
    if n not in a or n not in b:
        print(("ONLY IN tree " if n in b else "ONLY IN parent ") + dem[n])
        bad += 1
        continue
    (ra, ca), (rb, cb) = a[n], b[n]
    same_code = ca == cb
    key = (ra == rb, same_code)
    census[key] = census.get(key, 0) + 1
    if ra == rb and same_code:
        continue
    nd = sum(1 for op in difflib.SequenceMatcher(None, ca, cb, autojunk=False).get_opcodes() if op[0] != "equal"
             for _ in range(max(op[2] - op[1], op[4] - op[3])))
    oa, ob = occupancy(ra[0]), occupancy(rb[0])
    hard = ra[1] != rb[1] or ra[3:] != rb[3:] or ob < oa
    bad += hard
    rises += ob > oa
    print(f"{'FAIL ' if hard else 'RISE ' if ob > oa else ''}regs {ra} -> {rb}, occupancy {oa} -> {ob}, instr {len(ca)} -> {len(cb)}, differing lines {nd}: {dem[n]}")
for (sr, sc), k in sorted(census.items()):
    print(f"same_regs={sr} same_code={sc}: {k} kernels")
print(f"{len(a)} kernels in the parent, {len(b)} in the tree; {bad} FAIL, {rises} RISE")
sys.exit(1 if bad else 0)
