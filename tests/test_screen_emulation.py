"""The lane-local device code of the read screen, run on the host (tests/emul/screen_emul.cpp compiles the product's
csrc/vk_screen.h) against tests/screen_ref.py: every case of tests/screen_cases.py at two tile sizes and two unit sizes --
the windows, the distinct keys (every one of them), the table's size and every read's hits equal.  The program is
stand-alone (its own main): built once plainly and once with the address and undefined-behaviour sanitizers, run as a
program, never loaded into python.  Its header says what it does not cover (the kernels around the lane-local code: the
GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_cases as SC  # noqa: E402
import screen_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "screen_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
TILES = (SC.TILE, 128)
UNITS = (64, 16384)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("screen_emul")
    plain, san = str(d / "screen_emul"), str(d / "screen_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected():
    """Per case (fasta, k, slots asked, reads) and (status, windows, sorted keys, slots, hits): computed once, left
    unchanged.  The 1,000-key reference comes a second time with the table forced to 1,024 slots."""
    cases, want = [], []
    for c in SC.ALL_CASES:
        reads = [seq for text in c.samples for _, seq in R.split_records(text)[1]]
        keys = R.set_ints(c.fasta, c.k)
        windows = R.windows_ints(c.fasta, c.k)
        hits = [R.hits_ints(seq, keys, c.k) for seq in reads]
        for slots in (0, 1024) if c.name == "ref_1000_keys" else (0,):
            cases.append((c.name, c.fasta, c.k, slots, tuple(reads)))
            want.append((R.ref_status(c.fasta), windows, sorted(keys), slots or R.slots_for(windows), hits))
    return cases, want


def run(exe, d, cases, tile, unit):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, fasta, k, slots, reads in cases:
            f.write(struct.pack("<III", k, slots, len(fasta)) + fasta + struct.pack("<I", len(reads)))
            for r in reads:
                f.write(struct.pack("<I", len(r)) + r)
    r = subprocess.run([exe, src, dst, str(tile), str(unit)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, out = 0, []
    for case in cases:
        status, windows, distinct, slots = struct.unpack_from("<IQQQ", raw, at)
        at += 28
        keys = list(struct.unpack_from("<%dQ" % distinct, raw, at))
        at += 8 * distinct
        hits = list(struct.unpack_from("<%dI" % len(case[4]), raw, at))
        at += 4 * len(case[4])
        out.append((status, windows, keys, slots, hits))
    assert at == len(raw)
    return out


def check(cases, got, want):
    for (name, *_), g, w in zip(cases, got, want):
        assert g == w, name


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("tile", TILES)
def test_emulation_equals_the_rule(programs, tile, unit):
    cases, want = expected()
    check(cases, run(programs["plain"], programs["dir"], cases, tile, unit), want)


@pytest.mark.parametrize("tile", TILES)
def test_emulation_under_address_and_undefined_sanitizers(programs, tile):
    """No byte read past a text or a read, no probe past the table, no word read past the tile's; the same answers."""
    cases, want = expected()
    check(cases, run(programs["san"], programs["dir"], cases, tile, 64), want)
    check(cases, run(programs["san"], programs["dir"], cases, 4096, 256), want)
