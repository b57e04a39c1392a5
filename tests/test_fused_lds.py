"""Host-only: the LDS layout of the persistent tail kernel (FusedLds, altro-cpp_amd/csrc/altro_common.hpp).

k_sweep_fused takes the pointers of its LDS sub-blocks from FusedLds and Engine::PlanForwardLds takes the launch's LDS size
from FusedLds::bytes(): one description instead of pointer arithmetic in the kernel and a byte count in the engine that had
to agree by hand.  tests/cpp/fused_lds_driver.cpp is built against the header with plain g++ (it must not need HIP) and
prints, for a grid of shapes, every offset beside the byte count the engine computed before the struct existed (the formula
is copied literally into the driver).  Shapes: the built-in models and the shapes of tests/models/shape_chain.hpp at
N in {1, 2, 100, 126, 127}, and for (n, m) = (3, 2) every combination of N with rows in {0, 1, 7, 303} and nslots, npool in
{0, 1, 5}; element type double -- every engine, the fp32-record ones (WithRec32) included, keeps doubles in LDS -- and float
(four elements per 16 bytes: the other padding rule).
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fused_lds") / "fused_lds_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "fused_lds_driver.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def _id(c):
    return tuple(c[k] for k in ("type", "n", "m", "N", "rows", "nslots", "npool"))


def test_grid_is_complete(cases):
    ids = {_id(c) for c in cases}
    for t in ("double", "float"):
        for N in (1, 2, 100, 126, 127):
            for rows in (0, 1, 7, 303):
                for nslots in (0, 1, 5):
                    for npool in (0, 1, 5):
                        assert (t, 3, 2, N, rows, nslots, npool) in ids
            for n, m in ((3, 2), (6, 2), (12, 4), (1, 1), (2, 2), (1, 2), (3, 1), (5, 3), (7, 3), (9, 1), (13, 2), (6, 5), (3, 5)):
                assert (t, n, m, N, 7, 1, 5) in ids


def test_bytes_equal_the_former_formula(cases):
    for c in cases:
        assert c["bytes"] == c["parent"], _id(c)


def test_sub_blocks_are_aligned(cases):
    for c in cases:
        subs = {name: (off, size, align) for name, off, size, align in c["subs"]}
        for name, (off, size, align) in subs.items():
            assert off % align == 0, (_id(c), name, off, align)
        # the candidates keep the phase they had against the end of k_forward2's part of the layout (the gradient slots):
        # (4 + 2 + kBlock + 2 + 16) doubles behind it, 64 bytes into a 128-byte line
        assert subs["cand"][0] - subs["fh"][0] == (4 + 2 + 64 + 2 + 16) * 8
        assert (subs["cand"][0] - subs["fh"][0]) % 128 == 64


def test_sub_blocks_do_not_overlap(cases):
    for c in cases:
        subs = c["subs"]
        assert subs[0][1] == 0
        for (name, off, size, _), (nxt, off2, _, _) in zip(subs, subs[1:]):
            assert size >= 0 and off + size <= off2, (_id(c), name, nxt)
        name, off, size, _ = subs[-1]
        assert off + size <= c["used"] <= c["bytes"], (_id(c), name)
