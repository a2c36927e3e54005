"""The decisions of the inflate's host path (csrc/vk_gzplan.h) on the CPU: the fit of the chunk size against a table
computed with the rule as it stood inside vk_inflate_device (tests/golden/gz_chunk_fit.json), the chunk table,
the walk along every file's chain of chunks, the member checks, the CRC-32 operators.  The arrays a kernel would report are
written out by hand and the expectations follow from the rules: a chain must move forward inside its own file and end in
kGzEnd, a bad status counts only on a chunk the chain reaches, the size words must add up modulo 2^32, a sound chain whose
text does not fit is an overflow that reports the size it needs, anything else sends the file to the one-wavefront kernel,
and a file that is not accepted leaves no items behind."""
import json
import os
import zlib

import pytest

import gzplan_emul_lib as EM
from gzplan_emul_lib import END, GO_DIRECT, INFLATED, TOO_LARGE

HERE = os.path.dirname(os.path.abspath(__file__))
OVERFLOW, BAD_CRC = 8, 32
R = 62   # kGzMemRec


def test_constants():
    L = EM.load()
    assert (L.gzplan_mem_rec(), L.gzplan_chunk_min(), L.gzplan_big_file()) == (R, 1 << 17, 1 << 19)


# ---- chunk size ------------------------------------------------------------------------------------------------------
with open(os.path.join(HERE, "golden", "gz_chunk_fit.json")) as _f:
    FIT = json.load(_f)


def test_the_fit_table_holds_the_cases_it_should():
    names = [row["name"] for row in FIT]
    assert len(set(names)) == len(names) >= 40
    assert {row["fill"] for row in FIT} >= {0, 90, 96, 99, 100}
    assert {row["forced"] for row in FIT} >= {0, 1, 65536, 1 << 20}
    assert {row["num_cus"] for row in FIT} >= {4, 256, 304}
    assert all(row["chunk_waves"] == 24 for row in FIT)   # kGzChunkWaves: 4 SIMDs x VK_GZ_CHUNK_OCC, pinned by vk_inflate.h's static_assert


@pytest.mark.parametrize("row", FIT, ids=[row["name"] for row in FIT])
def test_chunk_size_is_what_it_was(row):
    assert EM.fit(row["lengths"], row["num_cus"] * row["chunk_waves"], row["forced"], row["fill"]) == row["chunk_bytes"]


def test_chunk_table():
    cb = 1 << 17
    offsets, lengths, caps = [0, 524288, 1224304], [524288, 700001, 1_000_000], [2_000_000, 100_000_000, 6_000_000]
    sym_total, chunk0, chunks = EM.table(cb, offsets, lengths, caps)
    # room per chunk: twice the file's ratio (at least 4) of a chunk's bytes, plus 65536, at most 2^25 elements
    room = [min(int(2.0 * max(c / n, 4.0) * cb) + 65536, 1 << 25) for c, n in zip(caps, lengths)]
    assert room == [8 * cb + 65536, 1 << 25, 12 * cb + 65536]
    counts = [4, 6, 8]
    assert chunk0 == [0, 4, 10] and len(chunks) == 18
    at = 0
    for f in range(3):
        for j in range(counts[f]):
            assert chunks[chunk0[f] + j] == {"in_off": offsets[f], "in_len": lengths[f], "out_off": at, "out_cap": room[f],
                                             "file_chunk0": chunk0[f], "nchunks": counts[f], "chunk_bytes": cb}
            at += room[f]
    assert sym_total == at
    assert EM.table(1 << 20, [0], [(1 << 20) + 1], [1 << 22])[1:] == ([0], [
        {"in_off": 0, "in_len": (1 << 20) + 1, "out_off": j * ((8 << 20) + 65536), "out_cap": (8 << 20) + 65536, "file_chunk0": 0,
         "nchunks": 2, "chunk_bytes": 1 << 20} for j in range(2)])


# ---- the chain walk --------------------------------------------------------------------------------------------------
def ch(sym_off, length, nxt, isize=0, status=0, members=(), nmem=None):
    d = {"sym_off": sym_off, "len": length, "next": nxt, "isize": isize, "status": status, "members": list(members)}
    if nmem is not None:
        d["nmem"] = nmem
    return d


def three(**last):
    """Chunks 0..2 of a file of 600 bytes in one member whose trailer chunk 2 records."""
    return [ch(0, 300, 1), ch(5000, 200, 2), ch(9000, 100, END, **{"isize": 600, "members": [(100, 0xAABBCCDD)], **last})]


REJECTED = {"items": [], "ok": [], "jobs": []}
G4 = 1 << 32
WALKS = {
    "a straight chain of three chunks": (
        EM.walk_case([(1000, 10_000, 3)], three()),
        {"verdict": [(INFLATED, 0, 600)], "items": [(0, 300, 1000), (5000, 200, 1300), (9000, 100, 1500)], "ok": [(0, 3, 0)],
         "jobs": [(1000, 600, 0, 0xAABBCCDD)]}),
    "a skipped chunk's bad status does not matter": (
        EM.walk_case([(1000, 600, 3)], [ch(0, 500, 2), ch(5000, 999, 2, isize=77, status=2, members=[(5, 1)]),
                                        ch(9000, 100, END, isize=600, members=[(100, 7)])]),
        {"verdict": [(INFLATED, 0, 600)], "items": [(0, 500, 1000), (9000, 100, 1500)], "ok": [(0, 2, 0)], "jobs": [(1000, 600, 0, 7)]}),
    "a bad status on a chunk the chain reaches": (
        EM.walk_case([(1000, 10_000, 3)], [ch(0, 300, 1), ch(5000, 200, 2, status=4), ch(9000, 100, END, isize=600)]),
        {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "a bad status on the first chunk": (
        EM.walk_case([(1000, 10_000, 1)], [ch(0, 600, END, isize=600, status=1)]), {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "next is the chunk itself": (
        EM.walk_case([(1000, 10_000, 3)], [ch(0, 300, 1), ch(5000, 200, 1), ch(9000, 100, END, isize=600)]),
        {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "next points backwards": (
        EM.walk_case([(1000, 10_000, 3)], [ch(0, 300, 1), ch(5000, 200, 0), ch(9000, 100, END, isize=600)]),
        {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "next points into the following file's chunks, and that file is accepted from item 0": (
        EM.walk_case([(1000, 10_000, 2), (20_000, 600, 2)],
                     [ch(0, 300, 1), ch(5000, 300, 2, isize=600), ch(10_000, 500, 3), ch(15_000, 100, END, isize=600, members=[(100, 9)])]),
        {"verdict": [(GO_DIRECT, 0, 0), (INFLATED, 0, 600)], "items": [(10_000, 500, 20_000), (15_000, 100, 20_500)], "ok": [(0, 2, 1)],
         "jobs": [(20_000, 600, 1, 9)]}),
    "the last chunk of a file may not point past the file": (
        EM.walk_case([(1000, 10_000, 3)], [ch(0, 300, 1), ch(5000, 200, 2), ch(9000, 100, 3, isize=600)]),
        {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "size words that do not add up": (
        EM.walk_case([(1000, 10_000, 3)], three(isize=599)), {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "size words that add up modulo 2^32, a text above 4 GiB": (
        EM.walk_case([(4096, 2 * G4, 3)], [ch(0, G4 // 2, 1), ch(5000, G4 // 2, 2), ch(9000, 5, END, isize=5, members=[(5, 0x1234)])]),
        # (no bound on the length here, unlike the one-wavefront path's files: see test_direct_files)
        {"verdict": [(INFLATED, 0, G4 + 5)], "items": [(0, G4 // 2, 4096), (5000, G4 // 2, 4096 + G4 // 2), (9000, 5, 4096 + G4)],
         "ok": [(0, 3, 0)], "jobs": [(4096, G4 + 5, 0, 0x1234)]}),
    "two files of one chunk, the second with a size word off by one": (
        EM.walk_case([(0, 1000, 1), (1000, 1000, 1)], [ch(0, 600, END, isize=600), ch(700, 600, END, isize=601)]),
        {"verdict": [(INFLATED, 0, 600), (GO_DIRECT, 0, 0)], "items": [(0, 600, 0)], "ok": [(0, 1, 0)], "jobs": []}),
    "a text larger than its room": (
        EM.walk_case([(1000, 599, 3)], three()), {"verdict": [(TOO_LARGE, OVERFLOW, 600)], **REJECTED}),
    "a text that just fits": (
        EM.walk_case([(1000, 600, 1)], [ch(40, 600, END, isize=600)]),
        {"verdict": [(INFLATED, 0, 600)], "items": [(40, 600, 1000)], "ok": [(0, 1, 0)], "jobs": []}),
    # the overflow is reported only for a chain that is sound: with both faults the file goes to the one-wavefront kernel
    # (which reports the overflow itself, without the size)
    "too large and size words that do not add up": (
        EM.walk_case([(1000, 599, 3)], three(isize=599)), {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "too large and a chain that turns back": (
        EM.walk_case([(1000, 100, 3)], [ch(0, 300, 1), ch(5000, 200, 1), ch(9000, 100, END, isize=600)]),
        {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "too large and a bad status behind it": (
        EM.walk_case([(1000, 100, 2)], [ch(0, 300, 1), ch(5000, 200, END, isize=500, status=8)]), {"verdict": [(GO_DIRECT, 0, 0)], **REJECTED}),
    "accepted, too large, rejected, accepted: the slices of the items follow one another": (
        EM.walk_case([(0, 1000, 2), (1000, 10, 3), (2000, 1000, 2), (3000, 1000, 2)],
                     [ch(0, 10, 1), ch(100, 20, END, isize=30),
                      ch(200, 5, 3), ch(300, 5, 4), ch(400, 5, END, isize=15),
                      ch(500, 7, 6), ch(600, 7, END, isize=15),
                      ch(700, 8, 8), ch(800, 9, END, isize=17, members=[(0, 0), (9, 5)])]),
        {"verdict": [(INFLATED, 0, 30), (TOO_LARGE, OVERFLOW, 15), (GO_DIRECT, 0, 0), (INFLATED, 0, 17)],
         "items": [(0, 10, 0), (100, 20, 10), (700, 8, 3000), (800, 9, 3008)], "ok": [(0, 2, 0), (2, 2, 3)],
         # (the member that ended with chunk 7's text is recorded by chunk 8 at its offset 0: the file's text up to 8)
         "jobs": [(3000, 8, 3, 0), (3008, 9, 3, 5)]}),
    "an empty member with a check word: the verdict carries the bad-CRC bit": (
        EM.walk_case([(0, 1000, 1)], [ch(0, 600, END, isize=600, members=[(600, 1), (600, 2)])]),
        {"verdict": [(INFLATED, BAD_CRC, 600)], "items": [(0, 600, 0)], "ok": [(0, 1, 0)], "jobs": [(0, 600, 0, 1)]}),
    "as many members in a chunk as it can record": (
        EM.walk_case([(50, 1000, 2)], [ch(0, R, 1, isize=R, members=[(k + 1, 100 + k) for k in range(R)]), ch(90, 3, END, isize=3, members=[(3, 9)])]),
        {"verdict": [(INFLATED, 0, R + 3)], "items": [(0, R, 50), (90, 3, 50 + R)], "ok": [(0, 2, 0)],
         "jobs": [(50 + k, 1, 0, 100 + k) for k in range(R)] + [(50 + R, 3, 0, 9)]}),
    "one member more than a chunk can record: accepted, not checked": (
        EM.walk_case([(50, 1000, 2)], [ch(0, R + 1, 1, isize=R + 1, members=[(k + 1, 100 + k) for k in range(R)], nmem=R + 1),
                                       ch(90, 3, END, isize=3, members=[(3, 9)])]),
        {"verdict": [(INFLATED, 0, R + 4)], "items": [(0, R + 1, 50), (90, 3, 51 + R)], "ok": [(0, 2, 0)], "jobs": []}),
    # (a count can disagree with the records only by exceeding them: also when the counts wrap around to 0)
    "member counts that disagree with the records": (
        EM.walk_case([(50, 1000, 2)], [ch(0, 10, 1, isize=10, members=[(10, 1)], nmem=1 << 31), ch(90, 3, END, isize=3, members=[(3, 9)], nmem=1 << 31)]),
        {"verdict": [(INFLATED, 0, 13)], "items": [(0, 10, 50), (90, 3, 60)], "ok": [(0, 2, 0)], "jobs": []}),
}

MEMBERS = {
    "three members, an empty one with check word 0": (
        EM.members_case(5, 4096, 1000, [(400, 0xA), (400, 0), (1000, 0xB)]), {"bits": 0, "jobs": [(4096, 400, 5, 0xA), (4496, 600, 5, 0xB)]}),
    "three members, an empty one with a check word": (
        EM.members_case(5, 4096, 1000, [(400, 0xA), (400, 3), (1000, 0xB)]), {"bits": BAD_CRC, "jobs": [(4096, 400, 5, 0xA), (4496, 600, 5, 0xB)]}),
    "an empty first member and an empty file": (
        EM.members_case(2, 64, 0, [(0, 0), (0, 1)]), {"bits": BAD_CRC, "jobs": []}),
    "a member that ends past the text: what was made so far is kept": (
        EM.members_case(5, 4096, 1000, [(400, 0xA), (1200, 0xB), (1300, 0xC)]), {"bits": 0, "jobs": [(4096, 400, 5, 0xA)]}),
    "a member that ends before the one in front, behind a bad empty one": (
        EM.members_case(5, 4096, 1000, [(0, 9), (400, 0xA), (300, 0xB), (1000, 0xC)]), {"bits": BAD_CRC, "jobs": [(4096, 400, 5, 0xA)]}),
    "no members": (EM.members_case(5, 4096, 1000, []), {"bits": 0, "jobs": []}),
}

# the one-wavefront path's files: checked when status 0, 1..kGzMemRec members, text below 4 GiB (its records' ends are 32-bit)
DIRECT = {
    "a file of two members": (EM.direct_case(3, 0, 2, 160, 1000, [(400, 1), (1000, 2)]), {"bits": 0, "jobs": [(160, 400, 3, 1), (560, 600, 3, 2)]}),
    "a file with a fault": (EM.direct_case(3, 4, 2, 160, 1000, [(400, 1), (1000, 2)]), {"bits": 0, "jobs": []}),
    "no member on record": (EM.direct_case(3, 0, 0, 160, 0, []), {"bits": 0, "jobs": []}),
    "more members than records": (EM.direct_case(3, 0, R + 1, 160, 1000, [(k + 1, k) for k in range(R)]), {"bits": 0, "jobs": []}),
    "as many members as records": (
        EM.direct_case(3, 0, R, 160, R, [(k + 1, k) for k in range(R)]), {"bits": 0, "jobs": [(160 + k, 1, 3, k) for k in range(R)]}),
    "a text of 4 GiB less one": (EM.direct_case(3, 0, 1, 0, G4 - 1, [(G4 - 1, 6)]), {"bits": 0, "jobs": [(0, G4 - 1, 3, 6)]}),
    "a text of 4 GiB": (EM.direct_case(3, 0, 1, 0, G4, [(0, 6)]), {"bits": 0, "jobs": []}),
    "an empty member with a check word": (EM.direct_case(3, 0, 1, 0, 0, [(0, 6)]), {"bits": BAD_CRC, "jobs": []}),
}
CASES = {**WALKS, **MEMBERS, **DIRECT}


@pytest.mark.parametrize("name", list(CASES))
def test_walks_and_member_checks(name):
    case, want = CASES[name]
    assert EM.run(case) == want


def test_the_same_cases_under_the_sanitizers(tmp_path):
    """The walk, member and direct cases through the stand-alone program built with -fsanitize=address,undefined: every
    array is as long as the case says and no longer, so a step past a chain's arrays is a step past an allocation."""
    exe = EM.sanitizer_program(str(tmp_path))
    got = EM.run_program(exe, [case for case, _ in CASES.values()], str(tmp_path))
    assert got == [want for _, want in CASES.values()]


# ---- CRC-32 operators ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 4032, 65535, 65536, 10 ** 6 + 7])
def test_crc_of_zero_bytes(n):
    assert EM.load().gzplan_crc_zeros(n) == zlib.crc32(b"\0" * n)
