"""The lane-local device code of the k-mer spectrum, run on the host (tests/emul/spectrum_emul.cpp compiles the product's
csrc/vk_spectrum.h) against tests/spectrum_ref.py: every well-framed sample of tests/spectrum_cases.py at two tile sizes
and every `every` of its case -- the whole row equal -- the table forced to 1,024 slots at about 900 distinct keys (long
probe chains, wrap-around at the table's end) and at about 1,100 (VK_SPEC_TABLE_FULL, and the program ends), and the
sample built to overflow its first table.  The program is stand-alone (its own main): built once plainly and once with
the address and undefined-behaviour sanitizers, run as a program, never loaded into python.  Its header says what it
does not cover (the kernels around the lane-local code: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_ref  # noqa: E402
import spectrum_cases as SC  # noqa: E402
import spectrum_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "spectrum_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
TILES = (SC.TILE, 4096)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("spectrum_emul")
    plain, san = str(d / "spectrum_emul"), str(d / "spectrum_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected():
    """Per well-framed sample (name, k, every, slots, reads) and (status, row): computed once, left unchanged."""
    samples, want = [], []
    runs = [(c, e, t) for c in SC.ALL_CASES + SC.FORCED_CASES for e in c.everys for t in c.samples]
    over = SC.overflow_sample()
    over_case = SC.Case("overflow", [over], 16, (64,), None)
    runs += [(over_case, 64, over), (over_case._replace(slots=4 * R.slots_for(len(over), 64)), 64, over)]
    for c, every, text in runs:
        status, recs = screen_ref.split_records(text)
        if status:
            continue
        slots = c.slots or R.slots_for(len(text), every)
        row, st = R.spectrum_numpy(text, c.k, every, slots)
        samples.append((c.name, c.k, every, slots, tuple(seq for _, seq in recs)))
        want.append((st, row.tolist()))
    assert [w[0] for s, w in zip(samples, want) if s[0] == "overflow"] == [R.VK_SPEC_TABLE_FULL, 0]
    return samples, want


def run(exe, d, samples, tile):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, k, every, slots, reads in samples:
            f.write(struct.pack("<IIII", k, every, slots, len(reads)))
            for r in reads:
                f.write(struct.pack("<I", len(r)) + r)
    r = subprocess.run([exe, src, dst, str(tile)], capture_output=True, text=True, timeout=120)   # (a probe that spins ends here)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    size = 4 + 8 * R.NSTAT
    assert len(raw) == size * len(samples)
    return [(struct.unpack_from("<I", raw, i * size)[0], list(struct.unpack_from("<%dQ" % R.NSTAT, raw, i * size + 4)))
            for i in range(len(samples))]


def check(samples, got, want):
    for (name, k, every, slots, _), g, w in zip(samples, got, want):
        assert g == w, (name, every, slots)


@pytest.mark.parametrize("tile", TILES)
def test_emulation_equals_the_rule(programs, tile):
    samples, want = expected()
    assert len(samples) > 70 and sum(1 for w in want if w[0] == R.VK_SPEC_TABLE_FULL) == 2
    check(samples, run(programs["plain"], programs["dir"], samples, tile), want)


@pytest.mark.parametrize("tile", TILES)
def test_emulation_under_address_and_undefined_sanitizers(programs, tile):
    """No probe past a table, no byte read past a read, no word read past the tile's; the same answers."""
    samples, want = expected()
    check(samples, run(programs["san"], programs["dir"], samples, tile), want)
