#!/usr/bin/env python3
"""Is every kernel of source tree B the same machine code as in source tree A?   (CPU only)

    tools/kernel_diff.py A B [--allow-removed NAME ...] [--keep DIR]

For every okvis2_amd/csrc/*.hip of either tree the device side is compiled with that tree's own
Makefile FLAGS (+ --cuda-device-only --no-gpu-bundle-output -c), once plain and once with
-DOKVFE_LAB, and compared per symbol:

  * the `llvm-objdump -d` text of the symbol with the "// address: encoding" comment stripped, and
  * the kernel's entry in the `llvm-readelf --notes` metadata (VGPRs, SGPRs, LDS, scratch, kernarg
    layout, ...), as text.

The requirement is equality.  Removing a kernel moves its neighbours, so ONE class of token is
masked: the PC-relative literal of the s_add_u32 / s_addc_u32 pair that follows an s_getpc_b64
(the distance to a global or to a function, which depends on what else the object holds).  Branch
offsets are relative to the instruction and are compared as they are.

A symbol may exist in A only if --allow-removed names it (a substring of the mangled name is
enough: `describe_extras_kernel`); no symbol may exist in B only.  Exit status 0 means: same
machine code, the set of kernels shrank by nothing but the allowed names.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join("okvis2_amd", "csrc")


def makefile_flags(tree):
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= *(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS = *(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()


def compile_device(tree, name, extra, out):
    cmd = [HIPCC, *makefile_flags(tree), *extra, "-x", "hip", "--cuda-device-only",
           "--no-gpu-bundle-output", "-c", os.path.join(tree, CSRC, name), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def disassembly(obj):
    """{symbol: [instruction text]} with the comment column stripped and the getpc literals masked"""
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", obj], check=True,
                          capture_output=True, text=True).stdout
    syms, cur, after_getpc = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
            after_getpc = 0
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()
        if ins.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc and re.match(r"s_addc?_u32 ", ins):
            ins = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", ins)
            after_getpc -= 1
        else:
            after_getpc = 0
        cur.append(ins)
    return syms


def metadata(obj):
    """{kernel symbol: its block of the amdhsa.kernels note, as text}"""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True,
                          capture_output=True, text=True).stdout
    kernels, block, inside = {}, None, False
    def close(b):
        if b:
            name = next(l.split(":", 1)[1].strip() for l in b if l.lstrip().startswith(".name:"))
            kernels[name] = [l for l in b if ".name:" not in l and ".symbol:" not in l]
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and line.startswith("  - "):
            close(block)
            block = [line]
        elif inside and line.startswith("    "):
            block.append(line)
        elif inside:
            close(block)
            block, inside = None, False
    close(block)
    return kernels


def short(sym):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    out = subprocess.run([filt, sym], capture_output=True, text=True).stdout.strip() if filt else ""
    out = out or sym
    return re.sub(r"\(.*", "", out.replace("okvfe::(anonymous namespace)::", "").replace("void ", ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="the source tree to compare against (the parent commit)")
    ap.add_argument("b", help="the source tree under test")
    ap.add_argument("--allow-removed", nargs="*", default=[], metavar="NAME")
    ap.add_argument("--keep", metavar="DIR", help="keep the objects here instead of a temporary directory")
    ap.add_argument("-j", type=int, default=8)
    args = ap.parse_args()
    names = sorted({f for t in (args.a, args.b) for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")})
    work = args.keep or tempfile.mkdtemp(prefix="kernel_diff_")
    os.makedirs(work, exist_ok=True)
    jobs = []
    for variant, extra in (("plain", []), ("lab", ["-DOKVFE_LAB"])):
        for name in names:
            for side, tree in (("a", args.a), ("b", args.b)):
                if os.path.exists(os.path.join(tree, CSRC, name)):
                    jobs.append((tree, name, extra, os.path.join(work, f"{side}_{variant}_{name}.o")))
    with ThreadPoolExecutor(args.j) as pool:
        list(pool.map(lambda j: compile_device(*j), jobs))

    bad = 0
    for variant in ("plain", "lab"):
        same = lines = 0
        removed, added, differ = [], [], []
        for name in names:
            objs = [os.path.join(work, f"{side}_{variant}_{name}.o") for side in "ab"]
            if not os.path.exists(objs[0]) or not os.path.exists(objs[1]):
                (removed if os.path.exists(objs[0]) else added).append(f"{name} (whole file)")
                continue
            (da, ma), (db, mb) = ((disassembly(o), metadata(o)) for o in objs)
            for sym in sorted(set(da) | set(db) | set(ma) | set(mb)):
                if sym not in db and sym not in mb:
                    removed.append(f"{name}: {short(sym)}")
                elif sym not in da and sym not in ma:
                    added.append(f"{name}: {short(sym)}")
                elif da.get(sym) != db.get(sym):
                    differ.append(f"{name}: {short(sym)} (code)")
                elif ma.get(sym) != mb.get(sym):
                    differ.append(f"{name}: {short(sym)} (metadata)")
                else:
                    same += 1
                    lines += len(da.get(sym, ()))
        unexpected = [r for r in removed if not any(n in r for n in args.allow_removed)]
        print(f"[{variant}] {same} symbols identical ({lines} instructions), {len(differ)} differ, "
              f"{len(removed)} removed ({len(unexpected)} not allowed), {len(added)} added")
        for tag, items in (("differs", differ), ("removed", removed), ("ADDED", added)):
            for it in items:
                print(f"    {tag}: {it}")
        bad += len(differ) + len(unexpected) + len(added)
    print("RESULT:", "same machine code" if bad == 0 else f"{bad} finding(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
