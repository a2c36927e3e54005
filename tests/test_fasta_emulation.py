"""The lane-local device code of the FASTA count, run on the host (tests/emul/fasta_emul.cpp compiles the product's
csrc/vk_fasta.h) against tests/fasta_ref.py: histograms, sequence bytes and statuses equal, for k = 5..9, at the unit
sizes the GPU tests use and at the smallest one.  The program is stand-alone (its own main): built once plainly and once
with the address and undefined-behaviour sanitizers, run as a program, never loaded into python.  Its header says what it
does not cover (the kernels' loads, scans and atomics: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_ref as FR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "fasta_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_emul")
    plain, san = str(d / "fasta_emul"), str(d / "fasta_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected(k, which):
    cases = FC.all_cases(k) if which == "all" else FC.small_cases(k) + FC.seam_cases(k, FC.SMALL_UNIT)[::5]
    return cases, [FR.count(data, k) for _, data in cases]


def run(exe, d, cases, k, unit):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, data in cases:
            f.write(struct.pack("<I", len(data)) + data)
    r = subprocess.run([exe, src, dst, str(k), str(unit)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = np.fromfile(dst, dtype=np.uint8)
    rec = 12 + 4 * 4 ** k
    assert raw.size == rec * len(cases)
    out = []
    for i in range(len(cases)):
        b = raw[i * rec:(i + 1) * rec]
        out.append((b[12:].view("<u4"), int(b[:4].view("<u4")[0]), int(b[4:12].view("<u8")[0])))
    return out


def check(cases, got, want):
    for (name, _), g, w in zip(cases, got, want):
        assert g[1] == w[1], name
        assert g[2] == w[2], name
        if w[1] == 0:
            assert np.array_equal(g[0], w[0]), name


@pytest.mark.parametrize("k", FC.KS)
@pytest.mark.parametrize("unit", (64, FC.SMALL_UNIT, FC.UNIT))
def test_emulation_equals_the_rule(programs, k, unit):
    cases, want = expected(k, "all")
    check(cases, run(programs["plain"], programs["dir"], cases, k, unit), want)


@pytest.mark.parametrize("k", (5, 9))
def test_emulation_on_the_unit_sized_sweeps(programs, k):
    cases = FC.seam_cases(k, FC.UNIT)[::4] + FC.span_seam_cases(k)[:2]
    want = [FR.count(data, k) for _, data in cases]
    check(cases, run(programs["plain"], programs["dir"], cases, k, FC.UNIT), want)


@pytest.mark.parametrize("k", FC.KS)
def test_emulation_under_address_and_undefined_sanitizers(programs, k):
    """No byte read before or past a sample, no shift out of range, the same answers."""
    cases, want = expected(k, "san")
    for unit in (64, FC.SMALL_UNIT):
        check(cases, run(programs["san"], programs["dir"], cases, k, unit), want)
