"""The host rules of the calls on record text (csrc/vk_textplan.h) on a CPU, through tests/emul/textplan_emul.cpp: the
workspace sizes against what the calls stated before the rules moved (tests/golden/text_ws.json), the layouts' pieces, the
record index of one-file samples against values written out here, what the argument rules refuse and the neighbour they
accept -- and the same cases through the sanitizer build."""
import json
import os

import pytest

import textplan_emul_lib as EM
from textplan_emul_lib import CHUNK, DEPTH, EMIT, QC, SCAN_BLOCK, SCREEN, SCREEN_BUILD, SPECTRUM, SPECTRUM_FASTA

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "text_ws.json")) as _f:
    WS = json.load(_f)["rows"]


def size_case(row):
    return EM.size_case(row["fn"], row.get("lengths", ()), row.get("records", ()), row.get("step_sample", ()), row.get("length", 0))


def align(n):
    return (n + 255) // 256 * 256


def sums_steps(items):
    """The 256-byte steps of a scan's `sums` piece that serves `items` items: a word per scan block and one more."""
    return align(8 * (-(-items // SCAN_BLOCK) + 1)) // 256


def totals(row):
    return sum(-(-x // CHUNK) for x in row["lengths"]), sum(row["records"])


# ---- the workspace sizes and the layouts ------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    assert {r["fn"] for r in WS} == set(range(7))
    text = [r for r in WS if r["fn"] in (SCREEN, SPECTRUM, DEPTH, QC)]
    for fn in (SCREEN, SPECTRUM, DEPTH, QC):
        mine = [r for r in text if r["fn"] == fn]
        assert {len(r["lengths"]) for r in mine} >= {0, 1, 2, 3}
        assert {x for r in mine for x in r["lengths"]} >= {0, 1, CHUNK - 1, CHUNK, CHUNK + 1}
        assert {x for r in mine for x in r["records"]} >= {0, 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1}
        # what tells a `sums` piece sized for max(chunks, records) from one sized for the chunks: records that take more
        # 256-byte steps of it than the chunks do -- and a shape the other way round, where both kinds agree
        assert any(sums_steps(totals(r)[1]) > sums_steps(totals(r)[0]) for r in mine)
        assert any(sums_steps(totals(r)[0]) > sums_steps(totals(r)[1]) for r in mine)
    # ... and the fixture does tell them apart: the screen's layout is the spectrum's with two pieces of records in place of
    # three of samples, so where the records take more steps of `sums` the difference shows
    by = {(r["fn"], r["name"].split(":")[1]): r["bytes"] for r in text}
    row = next(r for r in text if r["fn"] == SCREEN and r["name"].endswith(":records_over_chunks"))
    nchunks, nrec = totals(row)
    n = len(row["lengths"])
    tail_screen = align(8 * n) + align(8 * nrec) + align(8 * (nrec + 1))
    tail_spectrum = align(8 * (n + 1)) + 2 * align(8 * n)
    grown = 256 * (sums_steps(nrec) - sums_steps(nchunks))
    assert grown > 0
    assert by[(SCREEN, "records_over_chunks")] - tail_screen == by[(SPECTRUM, "records_over_chunks")] - tail_spectrum + grown
    emit = [r for r in WS if r["fn"] == EMIT]
    assert any(len(set(r["step_sample"])) < len(r["step_sample"]) for r in emit)          # a sample named twice
    assert any(s >= len(r["lengths"]) for r in emit for s in r["step_sample"])            # a step out of range
    items = lambda r: sum(r["records"][s] for s in r["step_sample"] if s < len(r["records"]))   # noqa: E731
    assert any(sums_steps(items(r)) > sums_steps(totals(r)[0]) for r in emit)
    assert any(sums_steps(totals(r)[0]) > sums_steps(items(r)) for r in emit)
    assert {r["length"] for r in WS if r["fn"] == SCREEN_BUILD} >= {0, 63, 64, 65}
    assert {x for r in WS if r["fn"] == SPECTRUM_FASTA for x in r["lengths"]} >= {0, 63, 64, 65}
    assert {len(r["lengths"]) for r in WS if r["fn"] == SPECTRUM_FASTA} >= {0, 1, 2, 3}


def check_layout(got, want_bytes):
    """The size is what the call stated before the rules moved; the pieces lie one after another in the stated order, each
    at a multiple of 256 bytes and clear of the next, and end at the total."""
    assert got["total"] == want_bytes
    at = 0
    for name, off, size in got["pieces"]:
        assert off == at and off % 256 == 0, name
        at += align(size)
    assert at == got["total"]


@pytest.mark.parametrize("row", WS, ids=[r["name"] for r in WS])
def test_workspace_size_and_layout(row):
    check_layout(EM.run(size_case(row)), row["bytes"])


# ---- the record index of one-file samples --------------------------------------------------------------------------------------
# an empty sample, one of one record, one whose budget (2) is below its records; the third spans three chunks
INDEX_CASE = EM.index_case([0, 16, 64], [0, 40, 2 * CHUNK + 5], [0, 1, 2])
INDEX_WANT = {
    "nchunks": 4, "nrec": 3,
    "rows": [dict(off=0, len=0, rec0=0, nrec=0, chunk0=0, chunk1=0),
             dict(off=16, len=40, rec0=0, nrec=1, chunk0=0, chunk1=1),
             dict(off=64, len=2 * CHUNK + 5, rec0=1, nrec=2, chunk0=1, chunk1=4)],
    "rec_base": [0, 0, 1, 3],
    "files": [dict(off=0, len=0, nrec=0, rec0=0, chunk0=0),
              dict(off=16, len=40, nrec=1, rec0=0, chunk0=0),
              dict(off=64, len=2 * CHUNK + 5, nrec=2, rec0=1, chunk0=1)],
    "fchunk": [0, 0, 1],
}


def test_record_index_of_one_file_samples():
    assert EM.run(INDEX_CASE) == INDEX_WANT
    assert EM.run(EM.index_case([], [], [])) == {"nchunks": 0, "nrec": 0, "rows": [], "rec_base": [0], "files": [], "fchunk": []}


# ---- refusals, each beside a neighbour that is accepted ---------------------------------------------------------------------
def refusal_case(call, args):
    return EM.check_case(call, **args)


def test_the_refusal_table_covers_what_it_should():
    names = [r[0] for r in EM.REFUSALS]
    assert len(set(names)) == len(names)
    for call in range(7):
        assert {r[3] for r in EM.REFUSALS if r[1] == call} >= {EM.VK_OK, EM.VK_EINVAL}
    assert [r[3] for r in EM.REFUSALS if "one 16-byte step short" in r[0]] == [EM.VK_ENOSPC, EM.VK_EINVAL]
    assert all(r[3] != EM.VK_OK for r in EM.REFUSALS if r[4])   # (what reaches an entry point returns before a launch)


@pytest.mark.parametrize("name", [r[0] for r in EM.REFUSALS])
def test_refusals(name):
    _, call, args, status, _ = next(r for r in EM.REFUSALS if r[0] == name)
    assert EM.run(refusal_case(call, args))["status"] == status


def test_block_plans():
    """The table plan and QC's: a sample's first workgroup, all of them last."""
    got = EM.run(EM.check_case(SPECTRUM, offsets=[0, 16, 32], nslots=[1024, 16384, 32768]))
    assert got == {"status": 0, "block_base": [0, 1, 2, 4]}
    got = EM.run(EM.check_case(SPECTRUM_FASTA, offsets=[0], nslots=[2 ** 20]))
    assert got == {"status": 0, "block_base": [0, 64]}
    got = EM.run(EM.check_case(QC, offsets=[0, 16, 32], records=[0, 1, 1025], per_block=512))
    assert got == {"status": 0, "block_base": [0, 0, 1, 4]}
    got = EM.run(EM.check_case(QC, offsets=[0, 16], records=[7, 8], per_block=4))
    assert got == {"status": 0, "block_base": [0, 2, 4]}


# ---- the same under the sanitizers ------------------------------------------------------------------------------------------
def test_the_same_cases_under_the_sanitizers(tmp_path):
    """The size, index and refusal cases through the stand-alone program built with -fsanitize=address,undefined: every
    array a rule reads is as long as the case says and no longer, and every piece of a layout lies inside a block of exactly
    the layout's size."""
    exe = EM.sanitizer_program(str(tmp_path))
    cases = [size_case(r) for r in WS] + [INDEX_CASE] + [refusal_case(r[1], r[2]) for r in EM.REFUSALS]
    got = iter(EM.run_program(exe, cases, str(tmp_path)))
    for row in WS:
        check_layout(next(got), row["bytes"])
    assert next(got) == INDEX_WANT
    for r in EM.REFUSALS:
        assert next(got)["status"] == r[3], r[0]
