"""The lane-local device code of `--qc-report`, run on the host (tests/emul/qc_emul.cpp compiles the product's
csrc/vk_qc.h) against tests/qc_ref.py: every stream of every case of tests/qc_cases.py, rows and status equal.  The
number of records between two merges of a workgroup's private counters is a compile-time constant (VK_QC_MERGE): the
program is built at the product's value and at 3.  It is stand-alone (its own main): built plainly and with the address
and undefined-behaviour sanitizers, run as a program, never loaded into python.  Its header says what it does not cover
(the kernels around the lane-local code: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qc_cases as QC  # noqa: E402
import qc_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "qc_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
MERGES = (None, 3)   # None: the product's


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("qc_emul")
    out = {"dir": d}
    for merge in MERGES:
        define = [] if merge is None else ["-DVK_QC_MERGE=%d" % merge]
        plain, san = str(d / ("qc_emul_%s" % merge)), str(d / ("qc_emul_san_%s" % merge))
        subprocess.check_call(["g++", "-O2", "-std=c++17"] + define + INCLUDES + [SRC, "-o", plain])
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                              define + INCLUDES + [SRC, "-o", san])
        out["plain", merge], out["san", merge] = plain, san
    return out


@functools.lru_cache(maxsize=None)
def expected():
    """Every stream of every case, and the rule's rows and status for them: computed once, left unchanged."""
    streams = [(c.name, i, text, n) for c in QC.all_cases() for i, (text, n) in enumerate(c.streams)]
    rows, status = R.rows([(text, n) for _, _, text, n in streams])
    rows.setflags(write=False)
    status.setflags(write=False)
    return streams, rows, status


def run(exe, d, streams):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, _, text, n in streams:
            f.write(struct.pack("<II", n, len(text)) + text)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = np.fromfile(dst, dtype=np.uint8).reshape(len(streams), 4 + 8 * R.NSTAT)
    return raw[:, 4:].copy().view(np.uint64), raw[:, :4].copy().view(np.uint32)[:, 0]


def check(streams, got, rows, status):
    for j, (name, i, _, _) in enumerate(streams):
        assert got[1][j] == status[j], (name, i)
        assert np.array_equal(got[0][j], rows[j]), (name, i, np.flatnonzero(got[0][j] != rows[j])[:8])


@pytest.mark.parametrize("merge", MERGES)
def test_emulation_equals_the_rule(programs, merge):
    streams, rows, status = expected()
    check(streams, run(programs["plain", merge], programs["dir"], streams), rows, status)


@pytest.mark.parametrize("merge", MERGES)
def test_emulation_under_address_and_undefined_sanitizers(programs, merge):
    """No byte read past a stream's end, no cell addressed past the tile; the same answers."""
    streams, rows, status = expected()
    check(streams, run(programs["san", merge], programs["dir"], streams), rows, status)
