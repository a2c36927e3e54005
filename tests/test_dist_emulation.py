"""The host-compilable device code of `compare`, run on the host (tests/emul/dist_emul.cpp compiles the product's
csrc/vk_dist.h: prep, slice folding, keys, per-row selection) against tests/dist_ref.py: every case of
tests/dist_cases.py, the matrix and the neighbours equal.  The matrix instruction is stood in by a plain loop.  The strip
height is a compile-time constant (VK_DIST_STRIP): the program is built at the product's value and at 64.  It is
stand-alone (its own main): built plainly and with the address and undefined-behaviour sanitizers, run as a program,
never loaded into python.  Its header says what it does not cover (the tile kernel's lanes: the GPU tests run those)."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dist_cases as DC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "dist_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
STRIPS = (None, 64)   # None: the product's


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dist_emul")
    out = {"dir": d}
    for strip in STRIPS:
        define = [] if strip is None else ["-DVK_DIST_STRIP=%d" % strip]
        plain, san = str(d / ("dist_emul_%s" % strip)), str(d / ("dist_emul_san_%s" % strip))
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + define + INCLUDES + [SRC, "-o", plain])
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                              define + INCLUDES + [SRC, "-o", san])
        out["plain", strip], out["san", strip] = plain, san
    return out


def run(exe, d, cases):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for c in cases:
            f.write(struct.pack("<IIIII", len(c.q), len(c.r), c.q.shape[1], c.n, 0 if c.qgroup is None else 1))
            f.write(c.q.tobytes() + c.r.tobytes())
            if c.qgroup is not None:
                f.write(c.qgroup.astype("<u4").tobytes() + c.rgroup.astype("<u4").tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = np.fromfile(dst, dtype=np.uint8)
    out, at = [], 0
    for c in cases:
        nq, nr, n = len(c.q), len(c.r), c.n
        m = raw[at:at + 8 * nq * nr].view(np.uint64).reshape(nq, nr)
        at += 8 * nq * nr
        idx = raw[at:at + 4 * nq * n].view(np.uint32).reshape(nq, n)
        at += 4 * nq * n
        d2 = raw[at:at + 8 * nq * n].view(np.uint64).reshape(nq, n)
        at += 8 * nq * n
        out.append((m, idx, d2))
    assert at == len(raw)
    return out


def check(cases, got):
    for c, (m, idx, d2) in zip(cases, got):
        em, eidx, ed2 = DC.expected(c.name)
        assert np.array_equal(m, em), (c.name, "matrix", np.argwhere(m != em)[:4])
        assert np.array_equal(idx, eidx), (c.name, "idx", np.argwhere(idx != eidx)[:4])
        assert np.array_equal(d2, ed2), (c.name, "d2", np.argwhere(d2 != ed2)[:4])


@pytest.mark.parametrize("strip", STRIPS)
def test_emulation_equals_the_rule(programs, strip):
    cases = DC.all_cases()
    check(cases, run(programs["plain", strip], programs["dir"], cases))


@pytest.mark.parametrize("strip", STRIPS)
def test_emulation_under_address_and_undefined_sanitizers(programs, strip):
    """No pixel read past an image, no entry addressed past a strip; the same answers."""
    cases = DC.all_cases()
    check(cases, run(programs["san", strip], programs["dir"], cases))


def test_the_extremes_need_the_slice():
    """The centred dot product of two black 512 x 512 images is 2^32: past an i32, so a whole row cannot stay in one."""
    c = DC.by_name("extremes_262144")
    m = DC.expected(c.name)[0]
    assert int(m[0, 1]) == DC.D2_BLACK_WHITE_512 and int(m[0, 0]) == 0
    s = c.q[0].astype(np.int64) - 128
    assert int(s @ s) == 2 ** 32
