#!/usr/bin/env python3
"""Every kernel of the PGD solver's units in a parent tree next to the same kernel in this tree: the check that moving device text between
translation units left the code objects alone.  No GPU: per unit a device-only compile with the flags of desc_amd/build.py, the gfx950 code
object unbundled, per kernel the resource fields of its metadata note, its code size and a hash of its code bytes.

    python tools/unit_kernels.py --parent <checkout of the parent commit> > profiles/pgd_units_kernels.txt

Exit status 1 if a kernel is missing, new, in two units, or differs in any field."""
import argparse
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from desc_amd.build import FLAGS  # noqa: E402

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
FIELDS = ["vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count",
          "max_flat_workgroup_size"]


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw).stdout


def kernels_of(root, unit, tmp):
    """{demangled kernel: [the FIELDS..., code bytes, sha256 of the code bytes (12 hex digits)]} of one unit of the tree at root."""
    base = os.path.join(tmp, re.sub(r"\W", "_", root + unit))
    hipcc = shutil.which("hipcc") or os.path.join(ROCM, "bin", "hipcc")
    flags = [f for f in FLAGS if f != "-shared"]
    run([hipcc] + flags + ["-I", os.path.join(root, "include"), "-I", os.path.join(root, "desc_amd", "csrc"), "--cuda-device-only", "-c",
                           os.path.join(root, "desc_amd", "csrc", unit), "-o", base + ".o"])
    run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950", "--input=" + base + ".o", "--output=" + base + ".co"])
    notes = run([os.path.join(LLVM, "llvm-readelf"), "--notes", base + ".co"])
    ks = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        blk = ".agpr_count:" + blk
        ks[re.search(r"\.name:\s*(\S+)", blk).group(1)] = [int(re.search(r"\.%s:\s*(\S+)" % k, blk).group(1)) for k in FIELDS]
    if not ks:
        return {}
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)", run([os.path.join(LLVM, "llvm-readelf"), "-SW", base + ".co"]))
    taddr = int(m.group(1), 16)
    run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", base + ".co", base + ".text"])
    with open(base + ".text", "rb") as f:
        text = f.read()
    for ln in run([os.path.join(LLVM, "llvm-readelf"), "-sW", base + ".co"]).splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[7] in ks and len(ks[f[7]]) == len(FIELDS):
            v, sz = int(f[1], 16), int(f[2])
            ks[f[7]] += [sz, hashlib.sha256(text[v - taddr:v - taddr + sz]).hexdigest()[:12]]
    names = list(ks)
    plain = run([shutil.which("c++filt") or os.path.join(LLVM, "llvm-cxxfilt")], input="\n".join(names)).split("\n")
    out = {}
    for n, d in zip(names, plain):
        d = re.sub(r"\(.*$", "", d.replace("void desc::", "").replace("desc::", "")).replace(", ", ",").replace("(bool)", "").replace("(int)", "")
        out[d] = ks[n]
    return out


def tree(root, units, tmp):
    with ThreadPoolExecutor(max_workers=min(8, len(units))) as ex:
        per_unit = list(ex.map(lambda u: kernels_of(root, u, tmp), units))
    where, twice = {}, []
    for u, ks in zip(units, per_unit):
        for k, v in ks.items():
            if k in where:
                twice.append(k)
            where[k] = (u, v)
    return where, twice


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="root of a checkout of the parent commit")
    ap.add_argument("--pattern", default="pgd*.hip,sweep_*.hip", help="units, as comma-separated globs under desc_amd/csrc")
    a = ap.parse_args()
    units_of = lambda root: sorted({os.path.basename(p) for g in a.pattern.split(",") for p in glob.glob(os.path.join(root, "desc_amd", "csrc", g))})
    with tempfile.TemporaryDirectory() as tmp:
        P, ptwice = tree(a.parent, units_of(a.parent), tmp)
        T, ttwice = tree(ROOT, units_of(ROOT), tmp)
    differ = [k for k in P if k in T and P[k][1] != T[k][1]]
    missing, new = sorted(set(P) - set(T)), sorted(set(T) - set(P))
    print("units of the parent: %s\nunits of this tree:  %s" % (" ".join(units_of(a.parent)), " ".join(units_of(ROOT))))
    print("%d kernels in the parent, %d in this tree; missing %s, new %s, in two units %s, differing %s" % (len(P), len(T), missing or "none", new or "none",
                                                                                                     sorted(ptwice + ttwice) or "none", sorted(differ) or "none"))
    print("fields: vgpr sgpr agpr, LDS bytes, scratch bytes, sgpr spills, vgpr spills, max workgroup size, code bytes, sha256 of the code bytes (12 digits)\n")
    fmt = lambda v: "%3d %3d %d %6d %4d %3d %2d %4d %6d %s" % tuple(v)
    print("%-34s %-17s %-17s %-56s %s" % ("kernel", "parent unit", "unit", "parent", "this tree"))
    for k in sorted(P, key=lambda k: (T.get(k, P[k])[0], k)):
        print("%-34s %-17s %-17s %-56s %s" % (k, P[k][0], T[k][0] if k in T else "-", fmt(P[k][1]), fmt(T[k][1]) if k in T else "-"))
    return 1 if (differ or missing or new or ptwice or ttwice) else 0


if __name__ == "__main__":
    sys.exit(main())
