"""The lane-local device code of the read-group split, run on the host (tests/emul/bam_groups_emul.cpp compiles the
product's csrc/vk_bam.h and csrc/vk_bam_groups.h) against tests/bam_groups_ref.py: every case of
bam_groups_cases.unit_cases at segment sizes 64, 256 and 4096 -- the note of every record, the text of every stream and
the statuses equal.  The program is stand-alone (its own main): built once plainly and once with the address and
undefined-behaviour sanitizers, run as a program, never loaded into python.  Its header says what it does not cover (the
LDS tables, shuffles and stores of the kernels: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_groups_cases as GC  # noqa: E402
import bam_groups_ref as GR  # noqa: E402
import bam_ref as BR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "bam_groups_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
SEGS = (64, 256, 4096)
NONE = 0xFFFF


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_groups_emul")
    plain, san = str(d / "bam_groups_emul"), str(d / "bam_groups_emul_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + INCLUDES + [SRC, "-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] +
                          INCLUDES + [SRC, "-o", san])
    return {"plain": plain, "san": san, "dir": d}


def streams_of(ids, pairs):
    """Every (select, group) of a file: all of its groups and the ungrouped reads, whole or split by class."""
    selects = (BR.SINGLE, BR.READ1, BR.READ2) if pairs else (BR.ALL,)
    return [(sel, g) for g in list(range(len(ids))) + [GR.UNGROUPED] for sel in selects]


@functools.lru_cache(maxsize=None)
def expected(exclude, pairs):
    """(cases as (name, bytes, first_record, ids, streams), per case (status, texts, notes)): computed once, left
    unchanged."""
    cases, want = [], []
    for name, data, ids in GC.unit_cases():
        first, _ = BR.header_end(data)
        streams = streams_of(ids, pairs)
        notes = []
        status, texts = GR.convert(data, first, ids, exclude, notes)
        at = {key: i for i, key in enumerate(streams)}
        local = [NONE if cls == 0 else at.get((cls if pairs else BR.ALL, g), NONE) for cls, g in notes]
        cases.append((name, data, first, tuple(ids), tuple(streams)))
        want.append((status, [texts.get(key, b"") for key in streams], [] if status else local))
    return cases, want


def run(exe, d, cases, seg, panel, exclude):
    src, dst = str(d / "in.bin"), str(d / "out.bin")
    with open(src, "wb") as f:
        for _, data, first, ids, streams in cases:
            f.write(struct.pack("<IQI", len(data), first, len(ids)))
            for i in ids:
                f.write(struct.pack("<I", len(i)) + i)
            f.write(struct.pack("<I", len(streams)) + b"".join(struct.pack("<II", s, g) for s, g in streams))
            f.write(data)
    r = subprocess.run([exe, src, dst, str(seg), str(panel), str(exclude)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    at, out = 0, []
    for case in cases:
        status, n = struct.unpack_from("<IQ", raw, at)
        at += 12
        notes = list(struct.unpack_from("<%dH" % n, raw, at))
        at += 2 * n
        walked, panels = struct.unpack_from("<QQ", raw, at)
        at += 16
        texts = []
        for _ in case[4]:
            (m,) = struct.unpack_from("<Q", raw, at)
            texts.append(raw[at + 8:at + 8 + m])
            at += 8 + m
        out.append((status, texts, notes, walked, panels))
    assert at == len(raw)
    return out


def check(cases, got, want):
    for (name, *_), (gs, gt, gn, walked, _), (ws, wt, wn) in zip(cases, got, want):
        assert gs == ws, name
        assert gn == wn, name
        assert gt == wt, name
        if not ws:
            assert walked == sum(1 for x in wn if x != NONE), name   # (every read has a stream here)


@pytest.mark.parametrize("pairs", (False, True))
@pytest.mark.parametrize("seg", SEGS)
def test_emulation_equals_the_rule(programs, seg, pairs):
    cases, want = expected(BR.EXCLUDE_DEFAULT, pairs)
    check(cases, run(programs["plain"], programs["dir"], cases, seg, GC.SMALL_PANEL, BR.EXCLUDE_DEFAULT), want)


def test_the_cases_say_what_they_should(programs):
    """The statuses of the bad cases, and that the walk is made for reads only."""
    cases, want = expected(BR.EXCLUDE_DEFAULT, False)
    got = dict(zip((c[0] for c in cases), run(programs["plain"], programs["dir"], cases, 256, GC.SMALL_PANEL, BR.EXCLUDE_DEFAULT)))
    for name in ("bad_type", "bad_subtype", "bad_subtype_A", "z_without_nul", "h_without_nul", "b_count_past_block", "b_count_huge",
                 "b_header_cut", "fixed_past_block", "stray_1", "stray_2"):
        assert got[name][0] == GR.BAD_AUX, name
    assert got["truncated_bad_aux"][0] == BR.TRUNCATED and got["bad_record_bad_aux"][0] == BR.BAD_RECORD
    assert got["ignored_bad"][0] == 0 and got["no_groups"][0] == 0
    reads = {c[0]: sum(1 for cls, _ in notes_of(c) if cls) for c in cases if c[0] in ("ignored_bad", "pairs")}
    assert got["ignored_bad"][3] == reads["ignored_bad"] and got["pairs"][3] == reads["pairs"]
    assert got["groups_1024"][4] > 50   # (panels of 3 segments of 256 bytes: many)


def notes_of(case):
    notes = []
    GR.convert(case[1], case[2], list(case[3]), BR.EXCLUDE_DEFAULT, notes)
    return notes


@pytest.mark.parametrize("seg", SEGS)
def test_emulation_under_address_and_undefined_sanitizers(programs, seg):
    """No byte read past a file or a table, none written past a text, the same answers; with panels of one segment and of
    a thousand, split by class, and with --bam-exclude 0xF00."""
    for exclude, pairs, panel in ((BR.EXCLUDE_DEFAULT, False, 1), (0xF00, True, GC.SMALL_PANEL), (BR.EXCLUDE_DEFAULT, True, 1000)):
        cases, want = expected(exclude, pairs)
        check(cases, run(programs["san"], programs["dir"], cases, seg, panel, exclude), want)
