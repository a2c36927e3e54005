"""The lane-local device code of `tree`, run on the host (tests/emul/tree_emul.cpp compiles the product's csrc/vk_tree.h and
csrc/vk_sketch.h with -ffp-contract=off) against tests/tree_ref.py, bit for bit: additive, noisy and arbitrary matrices of
3 to 257 leaves, each laid at an even and at an odd multiple of 8 bytes (the two places a row's 16-byte pairs can fall),
the tie matrices, every invalid matrix; 512 and 513 leaves, where an odd row's pairs reach the second column tile (its
lane 0 holds columns 511 and 512 and takes its R from the slot before the tile's own; at 512 leaves laid odd EVERY row is
odd and column 511 is met in the extra tile alone), as noise and as all ones (every step a tie across the tiles and
strips); 600 leaves with equal cherries in different tiles and strips (tree_cases.exact_cherries); and the per-block
walk of the pairs kernel on every pair of tests/sketch_cases.seam_pairs.  The program is stand-alone (its own main): built once plainly and once with the address
and undefined-behaviour sanitizers, run as a program, never loaded into python.  Its header says what it does not cover
(the kernels around the lane-local code: the GPU tests)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sketch_cases as SC  # noqa: E402
import tree_cases as TC  # noqa: E402
import tree_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "tree_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
PAIR_S = 64
CHERRIES_600 = ((3, 520), (17, 40), (530, 590))   # the winner in column tile 1, the others in tile 0 and in strip 33


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tree_emul")
    plain, san = str(d / "tree_emul"), str(d / "tree_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


@functools.lru_cache(maxsize=None)
def expected():
    """(matrices as (name, D, odd), what the rule gives each, pairs, what the loop gives each): computed once."""
    mats = [("additive_%d" % n, TC.additive(n, n)[0]) for n in (3, 4, 5, 8, 17, 64, 65)]
    mats += [("noisy_%d" % n, TC.noisy(n, 100 + n)) for n in (6, 40, 129, 257)]
    mats += [("arbitrary_%d" % n, TC.arbitrary(n, 200 + n)) for n in (7, 33)]
    mats += [("ones_%d" % n, TC.ones(n)) for n in (4, 9)] + [("three_identical", TC.three_identical())]
    mats += [("invalid_" + kind, TC.invalid(kind)) for kind in TC.INVALID]
    mats += [("noisy_%d" % n, TC.noisy(n, 100 + n)) for n in (512, 513)] + [("ones_513", TC.ones(513))]
    mats += [("exact_cherries_600", TC.exact_cherries(600, CHERRIES_600, 7))]
    runs = [(name, D, odd) for name, D in mats for odd in (0, 1)]
    want = {name: R.nj_np(D) for name, D in mats}
    for name, D in mats:
        if len(D) <= 40:
            st, nodes, lengths = R.nj_loop(D)
            assert st == want[name][0] and nodes == want[name][1].tolist(), name   # the two statements agree
            assert np.array(lengths).tobytes() == want[name][2].tobytes(), name
    st, nodes, lengths = want["exact_cherries_600"]
    assert st == 0 and tuple(nodes[:2].tolist()) == min(CHERRIES_600)         # of equal Q the smaller i, then the smaller j
    assert np.array_equal(lengths, np.round(lengths)) and lengths[:2].tolist() == [2.0, 4.0]   # integers throughout: real ties
    pairs = SC.seam_pairs(PAIR_S)
    return runs, want, pairs, [R.pair_blocks_loop(a, b, PAIR_S) for _, a, b in pairs]


def run(exe, d, runs, pairs):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, D, odd in runs:
            f.write(struct.pack("<III", 1, len(D), odd) + np.ascontiguousarray(D, dtype=np.float64).tobytes())
        for _, a, b in pairs:
            f.write(struct.pack("<IIII", 2, PAIR_S, len(a), len(b)) + np.array(a, dtype=np.uint64).tobytes() +
                    np.array(b, dtype=np.uint64).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, trees, got_pairs = 0, [], []
    for _, D, _ in runs:
        L = R.record_len(len(D))
        status = struct.unpack_from("<I", raw, at)[0]
        nodes = np.frombuffer(raw, dtype=np.uint32, count=L, offset=at + 4)
        lengths = np.frombuffer(raw[at + 4 + 4 * L:at + 4 + 12 * L], dtype=np.float64)
        trees.append((status, nodes, lengths))
        at += 4 + 12 * L
    for _ in pairs:
        both = np.frombuffer(raw, dtype=np.uint32, count=128, offset=at)
        got_pairs.append((both[:64].tolist(), both[64:].tolist()))
        at += 512
    assert at == len(raw)
    return trees, got_pairs


def check(got, exp):
    runs, want, pairs, pwant = exp
    trees, got_pairs = got
    for (name, D, odd), (status, nodes, lengths) in zip(runs, trees):
        w = want[name]
        assert status == w[0], (name, odd)
        assert np.array_equal(nodes, w[1]), (name, odd)
        assert lengths.tobytes() == w[2].tobytes(), (name, odd)   # bit for bit
        assert (status == R.BAD_VALUE) == name.startswith("invalid_"), name
    for (name, _, _), g, w in zip(pairs, got_pairs, pwant):
        assert g[0] == w[0] and g[1] == w[1], name


def test_emulation_equals_the_rule(programs):
    exp = expected()
    check(run(programs["plain"], programs["dir"], exp[0], exp[2]), exp)


def test_emulation_under_address_and_undefined_sanitizers(programs):
    """No pair read past a matrix, no walk past a sketch; the same answers."""
    exp = expected()
    check(run(programs["san"], programs["dir"], exp[0], exp[2]), exp)
