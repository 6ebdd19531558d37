#!/usr/bin/env python3
"""Every gfx950 kernel in the objects of two builds of the library, compared by name, without a
GPU (the static table of a kernel change: profiles/es_word/README.md):

    python3 tools/kdiff.py PARENT/ldpc_error_floor_amd/_build ldpc_error_floor_amd/_build

The objects are the build's own (its flags, the scheduler flags of the bit-sliced units included).
Per kernel: sha256 of the function's code bytes and the metadata fields VGPRs, SGPRs, VGPR / SGPR
spills, private segment, kernel-argument size, LDS and code size.  Prints the counts of identical,
changed, removed and new kernels and a line for each that is not identical.

A trailing ``, false`` of a k_bs / k_bsc template argument list is dropped from the second build's
names when that makes the name one of the first build's, so a template parameter added with a
default of false keeps the earlier builds comparable."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("vspill", "vgpr_spill_count"),
          ("sspill", "sgpr_spill_count"), ("priv", "private_segment_fixed_size"),
          ("karg", "kernarg_segment_size"), ("lds", "group_segment_fixed_size"))


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], capture_output=True, text=True)


def short_name(mangled):
    d = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    m = re.match(r"void (?:\w+::)*(\w+<[^>]*>)\(", d)          # (the argument type repeats the parameters)
    return m.group(1) if m else d


def kernels(build):
    """name -> fields, code size and code hash of every kernel in the objects of ``build``."""
    out = {}
    tmp = tempfile.mkdtemp(prefix="kdiff")
    for f in sorted(os.listdir(build)):
        if not f.endswith(".o"):
            continue
        fb, co = os.path.join(tmp, f + ".fb"), os.path.join(tmp, f + ".co")
        tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, os.path.join(build, f))
        if not os.path.exists(fb) or os.path.getsize(fb) == 0:
            continue                                              # host-only unit
        r = tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb,
                 "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co)
        if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
            raise SystemExit(f"{f}: no gfx950 code object\n{r.stderr}")
        meta = {}
        for e in tool("llvm-readelf", "--notes", co).stdout.split("\n  - ."):
            n = re.search(r"\.name:\s+(\S+)", e)
            if n and ".vgpr_count" in e:
                meta[n.group(1)] = {k: int((re.search(r"\." + y + r":\s+(\d+)", e) or [0, "-1"])[1]) for k, y in FIELDS}
        m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", tool("llvm-readelf", "-S", "-W", co).stdout)
        taddr, toff = int(m.group(1), 16), int(m.group(2), 16)
        data = open(co, "rb").read()
        for line in tool("llvm-readelf", "-s", "-W", co).stdout.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC" and p[7] in meta:
                at, size = toff + int(p[1], 16) - taddr, int(p[2])
                out[short_name(p[7])] = dict(meta[p[7]], code=size, sha=hashlib.sha256(data[at:at + size]).hexdigest()[:16])
    return out


def fmt(d):
    return "/".join(str(d[k]) for k in ("vgpr", "sgpr", "vspill", "sspill", "priv", "karg", "code"))


def main():
    a, b2 = kernels(sys.argv[1]), kernels(sys.argv[2])
    b = {}
    for n, v in b2.items():
        t = n[:-len(", false>")] + ">" if n.startswith("k_bs") and n.endswith(", false>") else n
        b[t if t in a and n not in a else n] = v
    same = [k for k in a if k in b and a[k] == b[k]]
    print(f"first build {len(a)} kernels, second {len(b)}: {len(same)} identical (code bytes and every field), "
          f"{sum(1 for k in a if k in b and a[k] != b[k])} changed, {sum(1 for k in a if k not in b)} removed, "
          f"{sum(1 for k in b if k not in a)} new")
    print("fields: VGPRs/SGPRs/VGPR spills/SGPR spills/private B/kernel arguments B/code B")
    for k in a:
        if k not in b:
            print("removed", k, fmt(a[k]))
        elif a[k] != b[k]:
            print("changed", k, fmt(a[k]), "->", fmt(b[k]), "(same code size, other bytes)" if a[k]["code"] == b[k]["code"] else "")
    for k in b:
        if k not in a:
            print("new    ", k, fmt(b[k]))


if __name__ == "__main__":
    main()
