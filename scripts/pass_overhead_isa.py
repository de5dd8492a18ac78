#!/usr/bin/env python3
"""Two builds of the library side by side, object by object: the resource lines of every kernel that holds the decision
loop, and whether the functions of the rules core are instruction-identical.

    python scripts/pass_overhead_isa.py <csrc/build of the parent commit> <csrc/build of this tree>

For every hot-kernel variant object, env_opp.o, vs_expert.o and env_after.o of the three record builds the gfx950 code
object is taken out of the host object (llvm-objdump --offloading).  Resources come from its metadata note (what
-Rpass-analysis=kernel-resource-usage prints, read per object so that a parallel build cannot mix them up); the
disassembly is cut into functions, kernel-name suffixes of the anonymous namespace and __hip_cuid_ normalised as in
scripts/isa_diff.sh, and every function whose name holds one of CORE is compared.  Exit status 1 if a core function differs."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
CORE = ["step_impl", "h_each_out", "h_after_out", "h_turn_out", "next_turn_out", "legal_mask_v", "ab_C_"]
KERNELS = ["k_play", "k_env_opp", "k_env_after"]   # k_play_vs matches k_play


def code_object(obj, tmp):
    dst = os.path.join(tmp, "x.o")
    subprocess.run(["cp", obj, dst], check=True)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "x.o"], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
    return os.path.join(tmp, "x.o.0.hipv4-amdgcn-amd-amdhsa--gfx950")


def functions(co):
    out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
    out = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", out)
    out = re.sub(r"_GLOBAL__N_[0-9]+", "_GLOBAL__N_", out)
    fns, name = {}, None
    for line in out.splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name = m.group(1)
            fns[name] = []
        elif name and line.strip():
            fns[name].append(re.sub(r"\s*//.*$", "", line))   # (the trailing comment is the address)
    return fns


def resources(co):
    out = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    rows = []
    for blk in out.split("- .agpr_count:")[1:]:
        def f(key):
            m = re.search(rf"\.{key}:\s*(\S+)", blk)
            return m.group(1) if m else "?"
        rows.append((f("name"), f("vgpr_count"), f("sgpr_count"), f("private_segment_fixed_size"), f("vgpr_spill_count"), f("sgpr_spill_count"),
                     f("group_segment_fixed_size")))
    return rows


def short(name):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    d = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip() if filt else name
    return re.sub(r"\(.*$", "", d.replace("(anonymous namespace)::", "")).replace("void ", "").replace("msbk::", "")


def main():
    old, new = sys.argv[1], sys.argv[2]
    rc = 0
    print("kernel resources, parent -> this tree: VGPRs, SGPRs, scratch bytes per lane, spilled VGPRs, spilled SGPRs, static LDS bytes")
    ident = []
    for b in ("std", "ext", "big"):
        objs = sorted(o for o in os.listdir(os.path.join(old, b)) if re.match(r"(variant_.*|env_opp|vs_expert|env_after)\.o$", o))
        for o in objs:
            with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
                ca, cb = code_object(os.path.join(old, b, o), ta), code_object(os.path.join(new, b, o), tb)
                ra = {r[0]: r[1:] for r in resources(ca)}
                rb = {r[0]: r[1:] for r in resources(cb)}
                for k in ra:
                    if any(s in k for s in KERNELS):
                        print(f"  {b}/{o:16s} {short(k):22s} {' '.join(f'{x:>5s}' for x in ra[k])}  ->  {' '.join(f'{x:>5s}' for x in rb.get(k, ()))}")
                fa, fb = functions(ca), functions(cb)
                core = sorted(n for n in fa if any(c in n for c in CORE))
                diff = [n for n in core if fa[n] != fb.get(n)]
                lines = sum(len(fa[n]) for n in core)
                ident.append(f"  {'DIFFERENT' if diff else 'SAME     '} {b}/{o:16s} {len(core)} core functions, {lines} instructions"
                             + (": " + ", ".join(short(n) for n in diff) if diff else ""))
                rc |= bool(diff)
    print("rules core (functions named " + ", ".join(c + "*" for c in CORE) + "), parent against this tree:")
    print("\n".join(ident))
    return rc


if __name__ == "__main__":
    sys.exit(main())
