#!/usr/bin/env python3
"""Compare the device code of two builds, symbol by symbol (reads digests and code-object metadata only).

  scripts/device_code_objects.sh <parent tree> <dir A>;  scripts/device_code_objects.sh <new tree> <dir B>
  python3 scripts/kernel_resource_diff.py <dir A> <dir B>

For every *.co of dir A: the symbols whose kernel_digest.py lines differ, and for each kernel among them the resources the
code object's metadata states (llvm-readelf --notes), A beside B: registers (unified vector file: arch + accumulation),
accumulation registers, scalar registers, private-segment (scratch) bytes per lane, static LDS bytes, code bytes, and the
waves per SIMD that the register count allows (512 registers per lane and SIMD, allocated in blocks of 8, at most 8
waves).  Kernel descriptors (<kernel>.kd) that differ only in the offset to their code are not listed.  Ends with a verdict
on the two conditions of a refactor: no kernel's scratch grows, none loses an occupancy step.
"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_digest import symbols  # noqa: E402

READELF = "/opt/rocm/llvm/bin/llvm-readelf"
FIELDS = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
          ("lds", ".group_segment_fixed_size"))


def metadata(path):
    out = subprocess.check_output([READELF, "--notes", path], text=True)
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", out)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(re.search(re.escape(f) + r":\s+(\d+)", block).group(1)) for k, f in FIELDS}
    return kernels


def digest(path):
    d = {}
    for line in open(path):
        name, size, sha = line.split()
        d[name] = (int(size), sha)
    return d


def waves(vgpr):
    return min(8, 512 // max(8, (vgpr + 7) // 8 * 8))


def demangle(name):
    s = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return re.sub(r"altro_hip::|altro_user::", "", re.sub(r"^void ", "", s)).split("(")[0]


def main(a, b):
    bad = []
    for co in sorted(f for f in os.listdir(a) if f.endswith(".co")):
        da, db = digest(os.path.join(a, co[:-3] + ".digest")), digest(os.path.join(b, co[:-3] + ".digest"))
        ma, mb = metadata(os.path.join(a, co)), metadata(os.path.join(b, co))
        sa, sb = ({n: (size, body) for n, size, body in symbols(os.path.join(d, co))} for d in (a, b))
        differ = sorted(n for n in set(da) | set(db) if da.get(n) != db.get(n))
        print("== %s: %d symbols, %d differ, %d of them kernels (the others: kernel descriptors)" % (
            co, len(set(da) | set(db)), len(differ), sum(1 for n in differ if n in ma)))
        for n in differ:
            if n not in da or n not in db:
                print("  %s: only in %s" % (demangle(n), "A" if n in da else "B"))
                bad.append(n)
                continue
            if n.endswith(".kd"):
                # a kernel descriptor holds the distance to its kernel's code (bytes 16 - 23), which moves whenever a
                # kernel in front of it changes size: a descriptor that differs in nothing else says nothing
                x, y = sa[n][1], sb[n][1]
                if n[:-3] not in differ and x[:16] + x[24:] != y[:16] + y[24:]:
                    print("  %s: descriptor of an unchanged kernel differs beyond its code offset" % demangle(n))
                    bad.append(n)
                continue
            if n not in ma:
                print("  %s: not a kernel" % demangle(n))
                continue
            ra, rb = dict(ma[n], code=da[n][0], waves=waves(ma[n]["vgpr"])), dict(mb[n], code=db[n][0], waves=waves(mb[n]["vgpr"]))
            print("  " + demangle(n))
            print("    " + "  ".join("%s %d -> %d" % (k, ra[k], rb[k]) for k in ("vgpr", "agpr", "sgpr", "scratch", "lds", "code", "waves")))
            if rb["scratch"] > ra["scratch"] or rb["waves"] < ra["waves"]:
                bad.append(n)
    print("VERDICT: " + ("no kernel's scratch grows, none loses an occupancy step" if not bad else "FAIL: " + " ".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
