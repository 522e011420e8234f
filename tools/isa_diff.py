"""Which kernels' machine code differs between two trees (CPU only: hipcc --cuda-device-only -S, the Makefile's
flags).  Each csrc/*.hip of both trees is compiled to device assembly and split per function symbol; comments and
directives are dropped, and the functions whose instruction streams differ are printed with their instruction
count and the resource fields of the code-object metadata, base -> new.
usage: python tools/isa_diff.py <base tree> [<new tree>]     (base: a git worktree of the parent commit)"""
import collections
import glob
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = "multi-modal-retrieval-predict-project_amd"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
          "group_segment_fixed_size")


def kernels(tree, name):
    """{symbol: (instruction lines, {metadata field: value})} of one source file"""
    src = os.path.join(tree, PKG, "csrc", name)
    asm = subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                          "-I" + os.path.join(tree, "include"), "-Wall", "-Wno-unused-function", "--cuda-device-only",
                          "-S", src, "-o", "-"], capture_output=True, text=True, check=True).stdout
    code, meta, cur, ent = {}, {}, None, None
    funcs = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M))
    for line in asm.splitlines():
        m = re.match(r"  - \.(\w+):\s+(\S+)", line) or (ent is not None and re.match(r"    \.(\w+):\s+(\S+)", line))
        if m:  # a kernel's entry of the metadata (its arguments' fields are indented deeper)
            ent = {} if line.startswith("  - ") else ent
            ent[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = ent
            continue
        m = re.match(r"(\S+):", line)
        if m and m.group(1) in funcs:
            cur = code.setdefault(m.group(1), [])
            continue
        text = line.split(";")[0].strip()
        if text.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and text and (not text.startswith(".") or text.endswith(":")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return {k: (v, meta.get(k, {})) for k, v in code.items()}


def main():
    base = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = sorted({os.path.basename(p) for t in (base, new) for p in glob.glob(os.path.join(t, PKG, "csrc", "*.hip"))})
    jobs = [(t, n) for n in names for t in (base, new) if os.path.exists(os.path.join(t, PKG, "csrc", n))]
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        res = dict(zip(jobs, ex.map(lambda j: kernels(*j), jobs)))
    differing = 0
    for n in names:
        b, w = res.get((base, n), {}), res.get((new, n), {})
        changed = [k for k in sorted(set(b) | set(w)) if b.get(k, ([],))[0] != w.get(k, ([],))[0]]
        differing += len(changed)
        print(f"{n}: {len(changed)} of {len(set(b) | set(w))} functions differ")
        for k in changed:
            (bi, bm), (wi, wm) = b.get(k, ([], {})), w.get(k, ([], {}))
            filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")  # readable names where one is installed
            name = subprocess.run([filt, k], capture_output=True, text=True).stdout.strip() if filt else k
            print(f"  {(name or k)[:150]}\n    instructions {len(bi)} -> {len(wi)}"
                  + "".join(f", {f} {bm.get(f, '-')} -> {wm.get(f, '-')}" for f in FIELDS))
            # the same opcodes in another order / other registers is scheduling; other opcodes (an fma where a
            # multiply and a subtract stood) is other arithmetic
            bo, wo = (collections.Counter(i.split()[0] for i in s if not i.endswith(":")) for s in (bi, wi))
            ops = ", ".join(f"{o} {bo[o]} -> {wo[o]}" for o in sorted(set(bo) | set(wo)) if bo[o] != wo[o])
            print(f"    opcodes: {ops or 'the same multiset'}")
    print(f"{differing} differing functions over {len(names)} files")
    return 0


if __name__ == "__main__":
    sys.exit(main())
