"""The lane-local device code of the per-window FASTA count, run on the host (tests/emul/fasta_windows_emul.cpp compiles
the product's csrc/vk_fasta_windows.h) against tests/fasta_windows_ref.py: every record's bases and the histogram of
every window equal, for k = 5 and 9 at units of 64 and 256 bytes and (N, S) = (100, 100), (96, 24), (64, 16).  The
program is stand-alone (its own main): built once plainly and once with the address and undefined-behaviour sanitizers,
run as a program, never loaded into python.  Its header says what it does not cover (the kernels' loads, scans, votes,
atomics, row ranges and the sum of tiles: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_ref as FR  # noqa: E402
import fasta_records_ref as RR  # noqa: E402
import fasta_windows_cases as WC  # noqa: E402
import fasta_windows_ref as WR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "fasta_windows_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
GEOMETRIES = ((100, 100), (96, 24), (64, 16))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_windows_emul")
    plain, san = str(d / "fasta_windows_emul"), str(d / "fasta_windows_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected(k, n, s):
    """(cases, per case (status, [bases of every record], [rows of every record])): computed once, left unchanged."""
    cases = WC.all_cases(n, s) + WC.batch(n, s)
    return cases, [(FR.status(d), [len(r) for r in RR.joined(d)], WR.rows(d, k, n, s)) for _, d in cases]


def run(exe, d, cases, k, unit, n, s):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, data in cases:
            f.write(struct.pack("<I", len(data)) + data)
    r = subprocess.run([exe, src, dst, str(k), str(unit), str(n), str(s)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, out = 0, []
    for _ in cases:
        status, nrec = struct.unpack_from("<II", raw, at)
        at += 8
        recs = []
        for _ in range(nrec):
            bases, nwin = struct.unpack_from("<QI", raw, at)
            at += 12
            rows = np.zeros((nwin, 4 ** k), dtype=np.uint32)
            for w in range(nwin):
                nnz, = struct.unpack_from("<I", raw, at)
                at += 4
                pairs = np.frombuffer(raw, dtype="<u4", count=2 * nnz, offset=at).reshape(nnz, 2)
                at += 8 * nnz
                rows[w, pairs[:, 0]] = pairs[:, 1]
            recs.append((bases, rows))
        out.append((status, recs))
    assert at == len(raw)
    return out


def check(cases, got, want):
    for (name, _), (gs, grecs), (ws, wbases, wrows) in zip(cases, got, want):
        assert gs == ws, name
        assert [b for b, _ in grecs] == wbases, name
        for r, ((_, g), w) in enumerate(zip(grecs, wrows)):
            assert g.shape == w.shape, (name, r)
            assert np.array_equal(g, w), (name, r, np.nonzero((g != w).any(axis=1))[0][:5])


@pytest.mark.parametrize("n,s", GEOMETRIES)
@pytest.mark.parametrize("unit", (64, 256))
@pytest.mark.parametrize("k", (5, 9))
def test_emulation_equals_the_rule(programs, k, unit, n, s):
    cases, want = expected(k, n, s)
    check(cases, run(programs["plain"], programs["dir"], cases, k, unit, n, s), want)


@pytest.mark.parametrize("n,s", GEOMETRIES)
@pytest.mark.parametrize("k", (5, 9))
def test_emulation_under_address_and_undefined_sanitizers(programs, k, n, s):
    """No byte read before or past a sample, no shift out of range, no tile past a record's, the same answers."""
    cases, want = expected(k, n, s)
    check(cases, run(programs["san"], programs["dir"], cases, k, 64, n, s), want)
    check(cases[::3], run(programs["san"], programs["dir"], cases[::3], k, 256, n, s), want[::3])
