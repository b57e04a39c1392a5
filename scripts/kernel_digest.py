#!/usr/bin/env python3
"""Digest of a gfx950 code object: one sorted line per FUNC / OBJECT symbol -- name, size, SHA-256 of the symbol's bytes.

Two builds whose digests are equal line for line hold the same device code (the same kernels, byte for byte), whatever
the host side of the translation unit looks like: the check of a host-only refactor.  __hip_cuid_* hashes the whole
translation unit and is left out.  Only bytes are hashed; no instruction is looked at.

  hipcc <the Makefile's CXXFLAGS> --cuda-device-only --no-gpu-bundle-output -c inst_x.hip -o inst_x.co
  python scripts/kernel_digest.py inst_x.co > inst_x.digest
"""
import hashlib
import re
import subprocess
import sys

READELF = "/opt/rocm/llvm/bin/llvm-readelf"


def symbols(path):
    """(name, size, bytes) of every FUNC / OBJECT entry of the code object's symbol tables"""
    data = open(path, "rb").read()
    out = subprocess.check_output([READELF, "-sW", "-S", path], text=True)
    sections = {}  # index -> (address, file offset, type)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S*)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", out, re.M):
        sections[int(m.group(1))] = (int(m.group(4), 16), int(m.group(5), 16), m.group(3))
    syms = []
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)", out, re.M):
        value, size, ndx, name = int(m.group(1), 16), int(m.group(2)), int(m.group(4)), m.group(5)
        if name.startswith("__hip_cuid_"):
            continue
        addr, off, kind = sections[ndx]
        syms.append((name, size, b"" if kind == "NOBITS" else data[off + value - addr:off + value - addr + size]))
    return syms


def digest(path):
    return sorted("%s %d %s" % (name, size, hashlib.sha256(body).hexdigest()) for name, size, body in symbols(path))


if __name__ == "__main__":
    for path in sys.argv[1:]:
        print("\n".join(digest(path)))
