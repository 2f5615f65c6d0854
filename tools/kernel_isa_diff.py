"""Generated code of the attention kernels of this tree against an earlier
copy of ray_amd/csrc (for instance `git archive` of the parent commit):

  python tools/kernel_isa_diff.py PARENT_CSRC_DIR [files...]
                                  [--rename OLD=NEW ...]

Each file (default: FILES below, hip/NAME.hip) is compiled for gfx950,
device only, from both trees; no GPU is needed. The name `ops` stands for
ops.hip, the whole extension as it is built: a shared DEV_INLINE function
is specialised for the arguments of all its callers in the translation
unit, so a kernel's code can differ between its own file and the extension.
Comments, directives and the __hip_cuid_* symbol are dropped and the
kernels paired by demangled name without the parameter list (c++filt; the
mangled name without it); --rename pairs a parent kernel with a kernel of
another name. Per kernel: the instruction count of both sides, the number
of differing lines, the register, LDS, scratch and spill figures of both
sides, and the differing lines themselves. It only diffs: what a
difference means is for the reader.
"""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["flash_attn_v5", "flash_attn_v7", "fa_bwd_v3", "fa_bwd_dq_v5",
         "fa_bwd_dkv_v6", "paged_attn_prefill"]
FIELDS = [".vgpr_count", ".sgpr_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size", ".vgpr_spill_count"]
# A kernel template that its file does not instantiate: the instances that
# ops.hip launches, named in a host function so that they are emitted.
USES = {"paged_attn_prefill": "void* isa_diff_uses[] = {" + ", ".join(
    f"(void*)&paged_attn_prefill_kernel<{d}, {w}, {f}>"
    for d in (64, 128) for w in (4, 8) for f in ("false", "true")) + "};\n"}
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def compile_asm(csrc, name, tmp, tag):
    src = os.path.join(tmp, f"{tag}_{name}.hip")
    out = os.path.join(tmp, f"{tag}_{name}.s")
    flags = [f"-I{csrc}", f"-I{os.path.join(csrc, 'hip')}"]
    if name == "ops":
        # the extension as ray_amd/csrc/build.py compiles it
        import sysconfig
        from torch.utils import cpp_extension
        src = os.path.join(csrc, "ops.hip")
        flags += ["-DTORCH_EXTENSION_NAME=_hip_ops", "-DUSE_ROCM=1",
                  "-DTORCH_API_INCLUDE_EXTENSION_H", "-fno-gpu-rdc",
                  "-Wno-unused-result"]
        flags += [f"-I{i}" for i in cpp_extension.include_paths()
                  + [sysconfig.get_paths()["include"]]]
    else:
        with open(src, "w") as f:
            f.write(f'#include "hip/{name}.hip"\n' + USES.get(name, ""))
    subprocess.check_call(
        [os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=gfx950",
         "--cuda-device-only", "-S", "-O3", "-std=c++17"] + flags
        + [src, "-o", out])
    with open(out) as f:
        return f.read()


def demangle(symbols):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not symbols or not filt:
        return {s: s for s in symbols}
    out = subprocess.check_output([filt] + symbols, text=True).split("\n")
    names = {}
    for sym, d in zip(symbols, out):
        d = d.split("(")[0]
        names[sym] = d[5:] if d.startswith("void ") else d
    return names


def kernels(asm):
    """{name: (instruction lines, {field: value})} of one assembly file."""
    meta = {}
    for entry in re.split(r"^  - (?=\.)", asm, flags=re.M)[1:]:
        sym = re.search(r"^\s+\.name:\s+(\S+)", entry, flags=re.M)
        if sym and ".vgpr_count:" in entry:
            meta[sym.group(1)] = {
                f: re.search(rf"^\s*{re.escape(f)}:\s+(\S+)", entry,
                             flags=re.M).group(1) for f in FIELDS}
    lines = asm.split("\n")
    body = {}
    for sym in meta:
        start = next(i for i, ln in enumerate(lines)
                     if ln.startswith(sym + ":"))
        ins = []
        for ln in lines[start + 1:]:
            ln = ln.split(";")[0].strip()
            if ln.startswith(".Lfunc_end"):
                break
            if not ln or "__hip_cuid_" in ln:
                continue
            if ln.startswith(".") and not ln.endswith(":"):
                continue  # directive
            # the label prefix counts the file's functions
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        body[sym] = ins
    names = demangle(list(meta))
    return {names[s]: (body[s], meta[s]) for s in meta}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_csrc")
    ap.add_argument("files", nargs="*", default=FILES)
    ap.add_argument("--rename", action="append", default=[],
                    metavar="OLD=NEW")
    args = ap.parse_args()
    rename = dict(r.split("=", 1) for r in args.rename)
    new_csrc = os.path.join(HERE, "ray_amd", "csrc")
    changed = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.files:
            old = kernels(compile_asm(args.parent_csrc, name, tmp, "parent"))
            new = kernels(compile_asm(new_csrc, name, tmp, "new"))
            print(f"== {name}.hip")
            for kn, (o_ins, o_meta) in old.items():
                nn = rename.get(kn, kn)
                if nn not in new:
                    print(f"{kn}: no kernel named {nn} in the new tree")
                    changed += 1
                    continue
                n_ins, n_meta = new.pop(nn)
                diff = [d for d in difflib.unified_diff(o_ins, n_ins, n=0,
                                                        lineterm="")
                        if not d.startswith(("---", "+++"))]
                n_diff = sum(not d.startswith("@@") for d in diff)
                count = sum(not i.endswith(":") for i in o_ins), \
                    sum(not i.endswith(":") for i in n_ins)
                changed += bool(n_diff) or o_meta != n_meta
                print(f"{kn}" + (f" -> {nn}" if nn != kn else ""))
                print(f"  instructions {count[0]} -> {count[1]}, "
                      f"{n_diff} differing lines")
                print("  " + ", ".join(
                    f"{f[1:]} {o_meta[f]} -> {n_meta[f]}" for f in FIELDS))
                for d in diff:
                    print("    " + d)
            for nn in new:
                print(f"{nn}: only in the new tree")
                changed += 1
    print(f"{changed} kernels differ")
    return 0


if __name__ == "__main__":
    sys.exit(main())
