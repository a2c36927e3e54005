"""The lane-local device code of the BAM to FASTQ conversion, run on the host (tests/emul/bam_emul.cpp compiles the
product's csrc/vk_bam.h) against tests/bam_ref.py: every case of bam_cases.unit_cases segment by segment, at segment sizes
64, 256 and 4096, with guesses and with VK_BAM_NO_GUESS -- texts of the four streams and statuses equal.  The program is
stand-alone (its own main): built once plainly and once with the address and undefined-behaviour sanitizers, run as a
program, never loaded into python.  Its header says what it does not cover (the ballots, scans, wave prefix sums and
stores of the kernels: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_cases as BC  # noqa: E402
import bam_ref as BR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "bam_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
SEGS = (64, 256, 4096)
SELECTS = (BR.ALL, BR.READ1, BR.READ2, BR.SINGLE)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_emul")
    plain, san = str(d / "bam_emul"), str(d / "bam_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected(exclude):
    """(cases with their first record and reference count, what the rule makes of each): computed once, left unchanged."""
    cases = [(name, data) + BR.header_end(data) for name, data in BC.unit_cases()]
    return cases, [BR.convert(data, first, exclude) for _, data, first, _ in cases]


def run(exe, d, cases, seg, no_guess, exclude):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, data, first, n_ref in cases:
            f.write(struct.pack("<IQi", len(data), first, n_ref) + data)
    r = subprocess.run([exe, src, dst, str(seg), str(int(no_guess)), str(exclude)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, out = 0, []
    for _ in cases:
        status, segments, rewalked = struct.unpack_from("<IQQ", raw, at)
        at += 20
        texts = {}
        for sel in SELECTS:
            (n,) = struct.unpack_from("<Q", raw, at)
            texts[sel] = raw[at + 8:at + 8 + n]
            at += 8 + n
        out.append((status, texts, segments, rewalked))
    assert at == len(raw)
    return out


def check(cases, got, want, seg, no_guess):
    for (name, data, _, _), (gs, gt, segments, rewalked), (ws, wt, _) in zip(cases, got, want):
        assert gs == ws, name
        assert gt == wt, name
        assert segments == max(1, -(-len(data) // seg)), name
        if no_guess and not ws:   # every segment but the first that starts a record is walked by the link pass
            assert rewalked <= segments - 1, name
    if no_guess:
        assert sum(r for _, _, _, r in got) > 0


@pytest.mark.parametrize("no_guess", (False, True))
@pytest.mark.parametrize("seg", SEGS)
def test_emulation_equals_the_rule(programs, seg, no_guess):
    cases, want = expected(BR.EXCLUDE_DEFAULT)
    check(cases, run(programs["plain"], programs["dir"], cases, seg, no_guess, BR.EXCLUDE_DEFAULT), want, seg, no_guess)


def test_the_decoy_is_guessed_and_rejected(programs):
    """With guesses at 256 bytes the decoy's segment guesses wrong and is walked again; the plain cases are not."""
    cases, _ = expected(BR.EXCLUDE_DEFAULT)
    got = dict(zip((c[0] for c in cases), run(programs["plain"], programs["dir"], cases, BC.SMALL_SEG, False, BR.EXCLUDE_DEFAULT)))
    assert got["decoy"][3] >= 1
    assert got["flags"][3] == 0 and got["first_1"][3] == 0


@pytest.mark.parametrize("no_guess", (False, True))
@pytest.mark.parametrize("seg", SEGS)
def test_emulation_under_address_and_undefined_sanitizers(programs, seg, no_guess):
    """No byte read past a file, none written past a text, no shift out of range, the same answers; also with
    --bam-exclude 0xF00."""
    for exclude in (BR.EXCLUDE_DEFAULT, 0xF00):
        cases, want = expected(exclude)
        check(cases, run(programs["san"], programs["dir"], cases, seg, no_guess, exclude), want, seg, no_guess)
