#!/usr/bin/env python3
"""Lists every kernel of every device unit of libpetiga_amd with a digest of its machine code, to check that a change of the
sources' layout left every kernel compiled as it was:

    python scripts/kernel_digest.py > after.txt         (the same in a checkout of the parent commit > before.txt)
    diff before.txt after.txt

A kernel's code here depends on what else is in its translation unit ("The units"), so the listing is per unit and in the
unit's order.  Each device unit of petiga_amd/build.py's UNITS is compiled with the build's flags plus --cuda-device-only -S.  One
line per kernel: the unit's object name, the mangled name, a digest of the text from the kernel's `.type NAME,@function` line to its
`.end_amdhsa_kernel` (comments dropped; of the local labels .LBB<n>_ and .Lfunc_end<n> only the function's number n normalised) and a
digest of the kernel's .amdhsa_ descriptor lines alone (registers, LDS, scratch).  Needs hipcc and no GPU.

    --root DIR   the checkout to list (default: the one this script is in)
    --keep DIR   keep the assembly files there
    --units a,b  only these objects (e.g. engine_main.o)"""
import argparse
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile


def kernels(asm):
    """(name, code digest, descriptor digest) of every kernel of an AMDGPU assembly text, in the text's order"""
    lines = asm.split("\n")
    type_line = {}
    out = []
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", ln)
        if m:
            type_line[m.group(1)] = i
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        body = []
        for raw in lines[type_line[name]:end + 1]:
            t = raw.split(";", 1)[0].strip()
            if t:
                body.append(re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", re.sub(r"\.LBB\d+_", ".LBB_", t)))
        desc = [t for t in body if t.startswith(".amdhsa_")]
        out.append((name, hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], hashlib.sha256("\n".join(desc).encode()).hexdigest()[:16]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--keep", default="")
    ap.add_argument("--units", default="")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("igx_build", os.path.join(args.root, "petiga_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    B.write_rtc_sources()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    tmp = args.keep or tempfile.mkdtemp(prefix="igx_digest_")
    os.makedirs(tmp, exist_ok=True)
    want = set(filter(None, args.units.split(",")))
    procs = []
    for obj, src, extra in B.UNITS:
        if not src.endswith(".hip") or (want and obj not in want):
            continue
        s = os.path.join(tmp, obj[:-2] + ".s")
        procs.append((obj, s, subprocess.Popen([hipcc] + B.FLAGS + extra + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", s],
                                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    rc = 0
    for obj, s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            print("hipcc failed for %s\n%s" % (obj, out[-4000:]), file=sys.stderr)
            rc = 1
            continue
        ks = kernels(open(s).read())
        for name, code, desc in ks:
            print(obj, name, code, desc)
        print("# %s: %d kernels" % (obj, len(ks)))
    if not args.keep:
        shutil.rmtree(tmp, ignore_errors=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
