"""The lane-local device code of the sketches, run on the host (tests/emul/sketch_emul.cpp compiles the product's
csrc/vk_sketch.h) against tests/sketch_ref.py: every hand-made table of tests/sketch_cases.py with the device's buffer and
run length and with a buffer of s + 16 in runs of 16 (more rounds, more merge levels), the table with one key in 7,000
slots (every round, the strict threshold), and every pair of tests/sketch_cases.seam_pairs.  The program is stand-alone
(its own main): built once plainly and once with the address and undefined-behaviour sanitizers, run as a program, never
loaded into python.  Its header says what it does not cover (the kernels around the lane-local code: the GPU tests)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sketch_cases as SC  # noqa: E402
import sketch_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "sketch_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
PAIR_S = 64


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sketch_emul")
    plain, san = str(d / "sketch_emul"), str(d / "sketch_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected():
    """(sketch runs as (table, cap, run), what the rule gives each, pairs, what the rule gives each): computed once."""
    runs, want = [], []
    for t in SC.hand_tables() + [SC.duplicate_table()]:
        ref = R.sketch_np(t.keys, t.counts, t.m, t.s)
        if t.name != "one_key_in_7000_slots":
            loop = R.sketch_loop(t.keys, t.counts, t.m, t.s)
            assert loop[0] == [int(x) for x in ref[0]] and loop[1] == ref[1], t.name   # the two statements agree
        for cap, run in ((SC.cap_of(len(t.keys), t.s), SC.RUN), (-(-(t.s + 16) // 16) * 16, 16)):
            runs.append((t, cap, run))
            want.append(ref)
    pairs = SC.seam_pairs(PAIR_S)
    pwant = [R.pair_loop(a, b, PAIR_S) for _, a, b in pairs]
    return runs, want, pairs, pwant


def run(exe, d, runs, pairs):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for t, cap, rn in runs:
            f.write(struct.pack("<IIIIIQ", 1, t.m, t.s, cap, rn, len(t.keys)) + t.keys.tobytes() + t.counts.tobytes())
        for _, a, b in pairs:
            f.write(struct.pack("<IIII", 2, PAIR_S, len(a), len(b)) + np.array(a, dtype=np.uint64).tobytes() +
                    np.array(b, dtype=np.uint64).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, sketches, passes, got_pairs = 0, [], [], []
    for _ in runs:
        eligible, length, npass = struct.unpack_from("<QQQ", raw, at)
        at += 24
        sketches.append((np.frombuffer(raw, dtype=np.uint64, count=length, offset=at), eligible))
        passes.append(npass)
        at += 8 * length
    for _ in pairs:
        got_pairs.append(struct.unpack_from("<II", raw, at))
        at += 8
    assert at == len(raw)
    return sketches, passes, got_pairs


def check(got, exp):
    runs, want, pairs, pwant = exp
    sketches, passes, got_pairs = got
    for (t, cap, rn), g, w, p in zip(runs, sketches, want, passes):
        assert g[1] == w[1] and np.array_equal(g[0], w[0]), (t.name, cap, rn)
        assert 2 <= p <= 7, (t.name, p)
    # which rounds ran, with the device's buffer: spread hashes take two passes, a shared prefix of 11 r bits r more
    by = {(t.name, rn): p for (t, cap, rn), p in zip(runs, passes)}
    assert by[("seam_spread", SC.RUN)] == 2 and by[("1024_slots_all_candidates", SC.RUN)] == 2
    assert [by[("seam_shared_top_%d" % b, SC.RUN)] for b in (11, 22, 33, 44)] == [3, 4, 5, 6]
    assert by[("one_key_in_7000_slots", SC.RUN)] == 7
    for (name, _, _), g, w in zip(pairs, got_pairs, pwant):
        assert tuple(g) == tuple(w), name


def test_emulation_equals_the_rule(programs):
    exp = expected()
    check(run(programs["plain"], programs["dir"], exp[0], exp[2]), exp)


def test_emulation_under_address_and_undefined_sanitizers(programs):
    """No read past a table, a sketch, a run or a buffer; the same answers."""
    exp = expected()
    check(run(programs["san"], programs["dir"], exp[0], exp[2]), exp)
