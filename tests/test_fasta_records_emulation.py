"""The lane-local device code of the per-record FASTA count, run on the host (tests/emul/fasta_records_emul.cpp compiles
the product's csrc/vk_fasta_records.h) against tests/fasta_records_ref.py: record counts, starts, bases, names and the
histogram of every record with a slot equal, for k = 5 and 9 at a unit of 256 bytes, with every record selected and with
every second one.  The program is stand-alone (its own main): built once plainly and once with the address and
undefined-behaviour sanitizers, run as a program, never loaded into python.  Its header says what it does not cover
(the kernels' loads, scans, votes and atomics: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_records_cases as RC  # noqa: E402
import fasta_records_ref as RR  # noqa: E402
import fasta_ref as FR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "fasta_records_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
UNIT = RC.SMALL_UNIT


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_records_emul")
    plain, san = str(d / "fasta_records_emul"), str(d / "fasta_records_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected(k):
    """(cases, per case (status, [(start, bases, name)], [histogram of every record])): computed once, left unchanged."""
    cases = RC.emulation_cases()
    return cases, [(FR.status(d), RR.table(d), [RR.count(r, k) for r in RR.joined(d)]) for _, d in cases]


def run(exe, d, cases, k, unit, sel):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, data in cases:
            f.write(struct.pack("<I", len(data)) + data)
    r = subprocess.run([exe, src, dst, str(k), str(unit), str(sel)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, out = 0, []
    for _ in cases:
        status, nrec = struct.unpack_from("<II", raw, at)
        at += 8
        recs = []
        for _ in range(nrec):
            start, bases = struct.unpack_from("<QQ", raw, at)
            name = raw[at + 16:at + 16 + RR.NAME_BYTES]
            slot, nnz = struct.unpack_from("<II", raw, at + 16 + RR.NAME_BYTES)
            at += 24 + RR.NAME_BYTES
            pairs = np.frombuffer(raw, dtype="<u4", count=2 * nnz, offset=at).reshape(nnz, 2)
            at += 8 * nnz
            hist = np.zeros(4 ** k, dtype=np.uint32)
            hist[pairs[:, 0]] = pairs[:, 1]
            recs.append((start, bases, name, slot, hist))
        out.append((status, recs))
    assert at == len(raw)
    return out


def check(cases, got, want, sel):
    for (name, _), (gs, grecs), (ws, wtable, whists) in zip(cases, got, want):
        assert gs == ws, name
        assert [g[:3] for g in grecs] == wtable, name
        nslots = 0
        for r, (g, wh) in enumerate(zip(grecs, whists)):
            if sel == 0 or r % 2 == 0:
                assert g[3] == nslots, name
                assert np.array_equal(g[4], wh), (name, r)
                nslots += 1
            else:
                assert g[3] == RR.NO_SLOT and not g[4].any(), (name, r)


@pytest.mark.parametrize("sel", (0, 1))
@pytest.mark.parametrize("k", (5, 9))
def test_emulation_equals_the_rule(programs, k, sel):
    cases, want = expected(k)
    check(cases, run(programs["plain"], programs["dir"], cases, k, UNIT, sel), want, sel)


@pytest.mark.parametrize("k", (5, 9))
def test_emulation_under_address_and_undefined_sanitizers(programs, k):
    """No byte read before or past a sample, no shift out of range, no row past the slots, the same answers."""
    cases, want = expected(k)
    check(cases, run(programs["san"], programs["dir"], cases, k, UNIT, 1), want, 1)
    check(cases[::4], run(programs["san"], programs["dir"], cases[::4], k, 64, 0), want[::4], 0)
