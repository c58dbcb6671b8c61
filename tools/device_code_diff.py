#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds kernel by kernel.

    tools/device_code_diff.py OLD_BUILD_DIR NEW_BUILD_DIR [--arch gfx950]

For every object file present in both directories (4c_amd/build of two checkouts) the gfx950 code
object is unbundled and disassembled, the instruction text of each kernel (addresses and encodings
stripped) is hashed, and the kernels are listed as same / changed / only in one build -- the check
that a change meant to add instantiations left the existing ones' instruction streams alone.
Exit code 1 when a kernel present in both builds differs.

    tools/device_code_diff.py OLD_BUILD_DIR NEW_BUILD_DIR --pool [--only fcg_amg,fcg_samg]

pools the kernels of every object of a build (--only: of the objects whose file name starts with one
of the prefixes) by mangled name and compares the two pools as one: the check for a change that moves
kernels between translation units.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def kernels_of(obj, arch, tmp):
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj],
        capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return None  # host-only object
    r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle",
        f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--input={fat}", f"--output={co}"],
        capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
        return None
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co],
        capture_output=True, text=True, check=True).stdout
    out, name, body = {}, None, []
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if name:
                out[name] = body
            name, body = m.group(1), []
        elif name and line.strip():
            t = line.split("//")[0].strip()
            t = re.sub(r"<[^>]*>", "<L>", t)  # branch targets by label, not address
            if t:
                body.append(t)
    if name:
        out[name] = body
    # the padding behind a kernel is no code: its length depends on what follows in the object (the
    # last kernel carries the section's fill), so a kernel that moves between objects would differ
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."):
            body.pop()
    return out


def pooled(build, arch, tmp, only):
    out = {}
    for f in sorted(os.listdir(build)):
        if not f.endswith(".o") or (only and not f.startswith(tuple(only))):
            continue
        for k, body in (kernels_of(os.path.join(build, f), arch, tmp) or {}).items():
            if k in out and out[k] != body:  # (a template's instantiation may be in several, alike)
                sys.exit(f"{build}: kernel {k} is in two objects with different code")
            out[k] = body
    return out


def compare(label, ko, kn):
    """Print the comparison of two {mangled name: instruction text}; returns the kernels changed."""
    demangle = lambda names: dict(zip(names, subprocess.run(["c++filt"] + list(names),
        capture_output=True, text=True).stdout.splitlines())) if names else {}
    dm = demangle(sorted(set(ko) | set(kn)))
    # an instantiation that only gained a defaulted trailing template argument `false`
    # (kernel<A, B> -> kernel<A, B, false>) is the same kernel under a new name
    old_by_dm = {dm[k]: k for k in ko}
    for k in list(kn):
        short = dm[k].replace(", false>(", ">(", 1)
        if k not in ko and short != dm[k] and short in old_by_dm and old_by_dm[short] not in kn:
            kn[old_by_dm[short]] = kn.pop(k)
    # a kernel whose argument struct grew keeps its code but reads the implicit arguments
    # behind the struct at a shifted offset: scalar loads that differ in the offset alone
    # ... and addresses its __constant__ tables relative to the program counter (s_getpc_b64 +
    # s_add_u32 with a literal), which moves with the code around it
    mask = lambda body: [re.sub(r"^(s_add_u32 s\d+, s\d+, )0x[0-9a-f]+$", r"\1OFF",
        re.sub(r"^(s_load_dword\w* .*, )0x[0-9a-f]+$", r"\1OFF", t)) for t in body]
    same = [k for k in ko if k in kn and ko[k] == kn[k]]
    moved = [k for k in ko if k in kn and ko[k] != kn[k] and mask(ko[k]) == mask(kn[k])]
    diff = [k for k in ko if k in kn and mask(ko[k]) != mask(kn[k])]
    added = [k for k in kn if k not in ko]
    gone = [k for k in ko if k not in kn]
    print(f"{label}: {len(same)} same, {len(moved)} same but for argument / pc-relative offsets, {len(diff)} changed, "
          f"{len(added)} added, {len(gone)} removed")
    for k in moved:
        n = sum(1 for x, y in zip(ko[k], kn[k]) if x != y)
        print(f"  offsets {dm[k]}  ({len(kn[k])} instructions, {n} offsets differ)")
    for k in diff:
        print(f"  CHANGED {dm[k]}  ({len(ko[k])} -> {len(kn[k])} instructions)")
    for k in added:
        h = hashlib.sha1("\n".join(kn[k]).encode()).hexdigest()[:10]
        print(f"  added   {dm[k]}  ({len(kn[k])} instructions, {h})")
    for k in gone:
        print(f"  removed {dm[k]}")
    return len(diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--pool", action="store_true", help="compare all kernels of a build by name, whatever object holds them")
    ap.add_argument("--only", default="", help="with --pool: comma-separated object file name prefixes")
    a = ap.parse_args()
    changed = 0
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        if a.pool:
            only = [p for p in a.only.split(",") if p]
            label = "pooled " + (", ".join(p + "*.o" for p in only) if only else "*.o")
            return 1 if compare(label, pooled(a.old, a.arch, t_old, only), pooled(a.new, a.arch, t_new, only)) else 0
        for f in sorted(os.listdir(a.new)):
            if not f.endswith(".o") or not os.path.exists(os.path.join(a.old, f)):
                continue
            ko = kernels_of(os.path.join(a.old, f), a.arch, t_old)
            kn = kernels_of(os.path.join(a.new, f), a.arch, t_new)
            if ko is None or kn is None:
                continue
            changed += compare(f, ko, kn)
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
