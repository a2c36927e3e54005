"""The lane-local device code of the depth filter, run on the host (tests/emul/depth_emul.cpp compiles the product's
csrc/vk_depth.h) against tests/depth_ref.py: every well-framed sample of tests/depth_cases.py at two tile sizes, every
`every` and every band of its case -- the whole row and the kept flag of every record equal -- the table forced to 1,024
slots at about 900 distinct keys and at about 1,100 (VK_SPEC_TABLE_FULL, a zero row, nothing kept), and the two probes
that only the emulation covers: a key absent from a table with free slots, and a key absent from a 1,024-slot table
without one (the walk ends after 1,024 probes).  The program is stand-alone (its own main): built once plainly and once
with the address and undefined-behaviour sanitizers, run as a program, never loaded into python.  Its header says what
it does not cover (the kernels around the lane-local code: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as DC  # noqa: E402
import depth_ref as D  # noqa: E402
import screen_ref  # noqa: E402
import spectrum_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "depth_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
TILES = (DC.TILE, 4096)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_emul")
    plain, san = str(d / "depth_emul"), str(d / "depth_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected():
    """Per well-framed sample (name, k, every, slots, lo, hi, reads) and (status, row, kept flags): computed once, left
    unchanged."""
    samples, want = [], []
    for c in DC.ALL_CASES + DC.FORCED_CASES:
        for every in c.everys:
            for bands in c.bandsets:
                for text, (lo, hi) in zip(c.samples, bands):
                    status, recs = screen_ref.split_records(text)
                    if status:
                        continue
                    slots = c.slots or R.slots_for(len(text), every)
                    _, row, st, flags = D.depth_count(text, c.k, every, lo, hi, slots)
                    reads = tuple(seq for _, seq in recs)
                    samples.append((c.name, c.k, every, slots, lo, hi, reads))
                    want.append((st, row.tolist(), flags if st == 0 else [False] * len(reads)))
    return samples, want


def run(exe, d, samples, tile):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, k, every, slots, lo, hi, reads in samples:
            f.write(struct.pack("<IIIIII", k, every, slots, lo, hi, len(reads)))
            for r in reads:
                f.write(struct.pack("<I", len(r)) + r)
    r = subprocess.run([exe, src, dst, str(tile)], capture_output=True, text=True, timeout=120)   # (a probe that spins ends here)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    got, at = [], 0
    for s in samples:
        status = struct.unpack_from("<I", raw, at)[0]
        row = list(struct.unpack_from("<%dQ" % D.NSTAT, raw, at + 4))
        at += 4 + 8 * D.NSTAT
        got.append((status, row, [bool(b) for b in raw[at:at + len(s[6])]]))
        at += len(s[6])
    assert at == len(raw)
    return got


def check(samples, got, want):
    for (name, k, every, slots, lo, hi, _), g, w in zip(samples, got, want):
        assert g == w, (name, every, slots, lo, hi)


@pytest.mark.parametrize("tile", TILES)
def test_emulation_equals_the_rule(programs, tile):
    samples, want = expected()
    assert len(samples) >= 240 and sum(1 for w in want if w[0] == D.VK_SPEC_TABLE_FULL) == 2
    check(samples, run(programs["plain"], programs["dir"], samples, tile), want)


@pytest.mark.parametrize("tile", TILES)
def test_emulation_under_address_and_undefined_sanitizers(programs, tile):
    """No probe past a table, no byte read past a read, no word read past the tile's, no bin past the histogram; the
    same answers."""
    samples, want = expected()
    check(samples, run(programs["san"], programs["dir"], samples, tile), want)


@pytest.mark.parametrize("which", ("plain", "san"))
def test_the_probes_for_absent_keys_end(programs, which):
    """a key absent from a table with free slots has depth 0; one absent from a 1,024-slot table without a free slot too,
    after 1,024 probes -- the walk ends, and under the sanitizers it reads no slot past the table"""
    r = subprocess.run([programs[which], "--probes"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", r.stderr[-2000:]
