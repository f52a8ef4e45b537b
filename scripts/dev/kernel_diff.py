#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    kernel_diff.py DIR_A DIR_B [--json OUT]

DIR_A / DIR_B hold device assembly, one `.s` per source, made with the Makefile's flags:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -S --cuda-device-only vrd_x.hip -o DIR/vrd_x.s

A kernel is matched across the two directories by its demangled template name (`local_attn_kernel<3, 16, true, 8>`), in whichever
file it was compiled: a kernel that moved to another translation unit is the same kernel.  Of each kernel the instruction stream
and the kernel descriptor (the `.amdhsa_*` lines) are compared, with label numbers, comments and file / line directives set aside.
Prints the kernels per file and those missing from DIR_B, new in DIR_B and different; exit status 1 if there are any.  It judges
nothing else about the instructions.
"""
import argparse
import json
import pathlib
import re
import shutil
import subprocess
import sys

KERNEL_RE = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
LABEL_NUM = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI|CPI)\d+(_\d+)?")
SKIP = (".file", ".loc", ".cfi_", ".p2align", ".ident", ".addrsig", ".section", ".type", ".size", ".globl", ".weak", ".protected", ".hidden", ".text")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def short_name(demangled):
    """`void (anonymous namespace)::k<3, true>(float const*, ...)` -> `k<3, true>`; the namespace `vrd::` stays."""
    s = demangled.replace("(anonymous namespace)::", "")
    s = re.sub(r"^void\s+", "", s)
    depth = 0
    for i, ch in enumerate(s):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i].strip()
    return s.strip()


def clean(line, names):
    line = line.split(";", 1)[0].strip()          # comments (no string literal in device code holds a ';' on these lines)
    if not line or line.startswith(SKIP):
        return None
    line = LABEL_NUM.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)      # .LBB84_12 -> .LBB_12
    if "_Z" in line:
        for mangled, short in names:
            if mangled in line:
                line = line.replace(mangled, short)
    return re.sub(r"\s+", " ", line)


def read_file(path):
    """{short name: (instruction lines, descriptor lines)} of one .s file"""
    lines = path.read_text().splitlines()
    mangled = [m.group(1) for m in map(KERNEL_RE.match, lines) if m]
    dem = demangle(mangled)
    shorts = {m: short_name(dem[m]) for m in mangled}
    order = sorted(shorts.items(), key=lambda kv: -len(kv[0]))      # longest first: one name may be a prefix of another
    kernels = {}
    label_at = {l.split(":", 1)[0]: i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l}
    desc_at = {KERNEL_RE.match(l).group(1): i for i, l in enumerate(lines) if KERNEL_RE.match(l)}
    for m in mangled:
        start = label_at[m]
        body = []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            c = clean(l, order)
            if c is not None:
                body.append(c)
        d0 = desc_at[m]
        desc = []
        for l in lines[d0 + 1:]:
            if l.strip() == ".end_amdhsa_kernel":
                break
            desc.append(re.sub(r"\s+", " ", l.strip()))
        if shorts[m] in kernels:
            raise SystemExit(f"{path}: two kernels reduce to the name {shorts[m]}")
        kernels[shorts[m]] = (body, desc)
    return kernels


def read_dir(d):
    per_file, where = {}, {}
    for path in sorted(pathlib.Path(d).glob("*.s")):
        ks = read_file(path)
        per_file[path.stem] = len(ks)
        for name, v in ks.items():
            if name in where:
                raise SystemExit(f"{d}: {name} is compiled in {where[name][0]} and in {path.stem}")
            where[name] = (path.stem, v)
    return per_file, where


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--json", help="also write the result to this file")
    a = ap.parse_args()
    files_a, ka = read_dir(a.dir_a)
    files_b, kb = read_dir(a.dir_b)
    missing = sorted(set(ka) - set(kb))
    new = sorted(set(kb) - set(ka))
    different, moved = [], []
    for name in sorted(set(ka) & set(kb)):
        (fa, (body_a, desc_a)), (fb, (body_b, desc_b)) = ka[name], kb[name]
        if fa != fb:
            moved.append(name)
        what = [w for w, x, y in (("instructions", body_a, body_b), ("descriptor", desc_a, desc_b)) if x != y]
        if what:
            different.append({"kernel": name, "file_a": fa, "file_b": fb, "differs_in": what})
    for label, files in (("A", files_a), ("B", files_b)):
        print(f"{label}: {sum(files.values())} kernels: " + ", ".join(f"{f} {n}" for f, n in files.items() if n))
    print(f"same name in both: {len(set(ka) & set(kb))}, of which in another file: {len(moved)}")
    print(f"missing from B: {len(missing)}, new in B: {len(new)}, different: {len(different)}")
    for n in missing:
        print(f"  missing   {n}  ({ka[n][0]})")
    for n in new:
        print(f"  new       {n}  ({kb[n][0]})")
    for d in different:
        print(f"  different {d['kernel']}  ({d['file_a']} -> {d['file_b']}): {', '.join(d['differs_in'])}")
    if a.json:
        pathlib.Path(a.json).write_text(json.dumps({"kernels_a": files_a, "kernels_b": files_b, "moved": len(moved), "missing": missing,
                                                    "new": new, "different": different}, indent=1) + "\n")
    return 1 if missing or new or different else 0


if __name__ == "__main__":
    sys.exit(main())
