"""The lane-local device code of the FASTA subsample ladder, run on the host (tests/emul/fasta_ladder_emul.cpp compiles
the product's csrc/vk_fasta_ladder.h) against tests/fasta_ladder_ref.py: histograms, taken bytes, sequence bytes and
statuses equal, for k = 5..9, at units of 64, 256 and 16384 bytes.  The program is stand-alone (its own main): built once
plainly and once with the address and undefined-behaviour sanitizers, run as a program, never loaded into python.  Its
header says what it does not cover (the kernels' loads, scans and atomics: tests/test_gpu_fasta_ladder.py runs those).

Cases: fasta_cases.small_cases(k) and every fifth of seam_cases(k, 256).  Steps: for every case three steps at each
fragment length k, k + 1, 64 and 150, dealt from the full product of thresholds, shifts and seeds
(fasta_ladder_ref.thinned) so that every combination comes up many times over the cases."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_ladder_ref as LR  # noqa: E402
import fasta_ref as FR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "fasta_ladder_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
PER_LENGTH = 3


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_ladder_emul")
    plain, san = str(d / "fasta_ladder_emul"), str(d / "fasta_ladder_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected(k):
    """(cases, the steps of each, [(status, bases, [(hist, taken)])]): computed once per k, shared, left unchanged."""
    cases = FC.small_cases(k) + FC.seam_cases(k, FC.SMALL_UNIT)[::5]
    by_len = [LR.thinned(k, L, len(cases), PER_LENGTH) for L in (k, k + 1, 64, 150)]
    steps = [sum((t[i] for t in by_len), []) for i in range(len(cases))]
    want = []
    for (_, data), ss in zip(cases, steps):
        st = FR.status(data)
        want.append((st, 0 if st else FR.bases(data), [LR.count(data, k, *s) for s in ss]))
    return cases, steps, want


def run(exe, d, cases, steps, k, unit):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for (_, data), ss in zip(cases, steps):
            f.write(struct.pack("<I", len(data)) + data + struct.pack("<I", len(ss)))
            for L, seed, thr, shift in ss:
                f.write(struct.pack("<IQQQ", L, seed, thr, shift))
    r = subprocess.run([exe, src, dst, str(k), str(unit)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, out = 0, []
    for ss in steps:
        status, bases = struct.unpack_from("<IQ", raw, at)
        at += 12
        got = []
        for _ in ss:
            taken, n = struct.unpack_from("<QI", raw, at)
            at += 12
            bins = np.frombuffer(raw, dtype="<u4", count=2 * n, offset=at).reshape(n, 2)
            at += 8 * n
            hist = np.zeros(4 ** k, dtype=np.uint32)
            hist[bins[:, 0]] = bins[:, 1]
            got.append((hist, taken))
        out.append((status, bases, got))
    assert at == len(raw)
    return out


def check(cases, steps, got, want):
    for (name, _), ss, g, w in zip(cases, steps, got, want):
        assert g[0] == w[0] and g[1] == w[1], name
        for s, (gh, gt), (wh, wt) in zip(ss, g[2], w[2]):
            assert gt == wt, (name, s)
            assert np.array_equal(gh, wh), (name, s)


@pytest.mark.parametrize("k", FC.KS)
@pytest.mark.parametrize("unit", (64, FC.SMALL_UNIT, FC.UNIT))
def test_emulation_equals_the_rule(programs, k, unit):
    cases, steps, want = expected(k)
    check(cases, steps, run(programs["plain"], programs["dir"], cases, steps, k, unit), want)


@pytest.mark.parametrize("k", FC.KS)
def test_emulation_under_address_and_undefined_sanitizers(programs, k):
    """No byte read before or past a sample, no shift or index out of range, the same answers."""
    cases, steps, want = expected(k)
    for unit in (64, FC.SMALL_UNIT, FC.UNIT):
        check(cases, steps, run(programs["san"], programs["dir"], cases, steps, k, unit), want)
