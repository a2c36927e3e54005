"""The rule of `--from-fasta --per-record` on the CPU ("--from-fasta --per-record"): the two statements
of tests/fasta_records_ref.py agree, the records' bases and rows sum to the sample's (fasta_ref.count, fasta_ref.bases),
and the host's naming (fasta.record_names), planning (fasta.record_plan), label lookup and command-line refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_records_cases as RC  # noqa: E402
import fasta_records_ref as RR  # noqa: E402
import fasta_ref as FR  # noqa: E402

from varkoder_amd.fasta import RECORD_HIST_BYTES, SAMPLED_HIST_BYTES, RecordLabels, record_names, record_plan  # noqa: E402

CASES = (RC.seam_cases_small()[::7] + RC.many_cases() + RC.slot_batch() + RC.batch_cases() + FC.header_cases(7) + FC.line_cases(7)[::3])


def test_the_two_statements_agree():
    """One record per header line, in order, also without sequence bytes; none for a bad start or an empty sample; the
    walk's start is a '>' at a line start and its name the header line behind it."""
    for name, data in CASES:
        recs, found = RR.joined(data), RR.walk(data)
        assert len(recs) == len(found), name
        if FR.status(data) or not data:
            assert recs == [] and found == [], name
            continue
        assert found[0][0] == 0, name
        for start, nm in found:
            assert data[start:start + 1] == b">" and (start == 0 or data[start - 1:start] == b"\n"), name
            assert data[start + 1:start + 1 + len(nm)] == nm and b"\n" not in nm, name
            assert data[start + 1 + len(nm):start + 2 + len(nm)] in (b"\n", b""), name
        assert len(found) == sum(1 for ln in data.split(b"\n") if ln.startswith(b">")), name
        for (_, _, kept), (_, nm) in zip(RR.table(data), found):
            assert len(kept) == RR.NAME_BYTES and kept.rstrip(b"\0") == nm[:RR.NAME_BYTES].rstrip(b"\0"), name


@pytest.mark.parametrize("k", (5, 7, 9))
def test_sum_invariants(k):
    """The bases of a sample's records sum to its bases, their rows (mod 2^32) to its row."""
    for name, data in CASES:
        if FR.status(data):
            continue
        recs = RR.joined(data)
        assert sum(len(r) for r in recs) == FR.bases(data), name
        total = np.zeros(4 ** k, dtype=np.uint64)
        for r in recs:
            total += RR.count(r, k)
        assert np.array_equal((total & 0xFFFFFFFF).astype(np.uint32), FR.count(data, k)[0]), name


def test_record_names():
    names, dup = record_names("f", [b"NC_1.2 Homo sapiens", b"a\tb", b"x\r", b"c@d+e/f|g", b"ok.-_09AZaz", b"", b" lead", b"\tt",
                                    b"\xc3\xa9t\xc3\xa9"])
    assert names == ["f__NC_1.2", "f__a", "f__x", "f__c_d_e_f_g", "f__ok.-_09AZaz", "f__record6", "f__record7", "f__record8", "f__" + "__t__"]
    assert dup == []
    names, dup = record_names("s.v2", [b"q" * 100, b"q" * 101, b"q" * 99 + b" q", b"q" * 100 + b"\r"])
    assert names == ["s.v2__" + "q" * 100, "s.v2__" + "q" * 100, "s.v2__" + "q" * 99, "s.v2__" + "q" * 100] and dup == [1, 3]
    names, dup = record_names("f", [b"a", b"b", b"a x", b"a\r", b"", b"record5", b"B"])
    assert names == ["f__a", "f__b", "f__a", "f__a", "f__record5", "f__record5", "f__B"] and dup == [2, 3, 5]
    assert record_names("f", []) == ([], [])


def test_record_plan():
    assert RECORD_HIST_BYTES == SAMPLED_HIST_BYTES == 1 << 30
    bases = [5000, 10, 1000, 999, 1001, 7000, 0, 1000, 2500]
    chosen = [i for i, b in enumerate(bases) if b >= 1000]
    for ncode, budget in ((4 ** 7, 3 * 4 * 4 ** 7), (4 ** 9, 2 * 4 * 4 ** 9 + 17), (4 ** 5, 1 << 30)):
        calls = record_plan(bases, 1000, budget, ncode)
        assert [g for c in calls for g in c] == chosen   # consecutive runs that cover exactly the selected records
        assert all(c and len(c) * 4 * ncode <= budget for c in calls)
        assert all(len(c) == budget // (4 * ncode) for c in calls[:-1])
    assert record_plan(bases, 1000, 4 * 4 ** 7, 4 ** 7) == [[g] for g in chosen]      # a budget of one row
    assert record_plan(bases, 1000, 1, 4 ** 9) == [[g] for g in chosen]               # a single row always fits
    assert len(record_plan(bases, 1000, ncode=4 ** 7)) == 1 and len(record_plan([1000] * 5000, 1000, ncode=4 ** 9)) == 5
    for min_len, want in ((999, [0, 2, 3, 4, 5, 7, 8]), (1000, [0, 2, 4, 5, 7, 8]), (1001, [0, 4, 5, 8])):   # bases - 1, bases, bases + 1
        assert [g for c in record_plan(bases, min_len, 1 << 30, 4 ** 7) for g in c] == want
    assert record_plan([], 1000) == [] and record_plan([5, 6], 1000) == []
    assert record_plan(np.array(bases, dtype=np.uint64), 1000, 1 << 30, 4 ** 7) == [chosen]


def test_labels_by_record_then_by_file():
    lab = RecordLabels({"coll": ["family:A"], "coll__r2": ["genus:B"], "a": ["x"], "a__b": ["y"]}, ["coll", "asm", "a", "a__b"])
    assert lab.get("coll__r1", []) == ["family:A"] and lab.get("coll__r2", []) == ["genus:B"]
    assert lab.get("asm__c1", []) == [] and lab.get("coll", []) == ["family:A"]
    assert lab.get("a__b__c", []) == ["y"] and lab.get("a__c", []) == ["x"]
    assert RecordLabels(None, ["f"]).get("f__r", []) == []


@pytest.mark.parametrize("argv", [
    ["image", "in", "--per-record"],
    ["image", "in", "--min-record-length", "2000"],
    ["image", "in", "--from-fasta", "--min-record-length", "2000"],
    ["image", "in", "--from-raw", "--per-record"],
    ["image", "in", "--from-fasta", "--per-record", "--fragments"],
    ["image", "in", "--from-fasta", "--per-record", "--min-record-length", "6"],
    ["image", "in", "--from-fasta", "--per-record", "-k", "9", "--min-record-length", "8"],
    ["query", "in", "out", "-l", "m", "--vocab", "v", "--per-record"],
    ["query", "in", "out", "-l", "m", "--vocab", "v", "--min-record-length", "2000"],
    ["query", "in", "out", "-l", "m", "--vocab", "v", "--from-fasta", "--per-record", "--min-record-length", "6"],
])
def test_cli_refusals(argv):
    from varkoder_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2


def test_cli_accepts():
    from varkoder_amd import cli
    a = cli.parse_args(["image", "in", "--from-fasta", "--per-record", "--min-record-length", "7"])
    assert a.per_record and a.min_record_length == 7
    a = cli.parse_args(["query", "in", "out", "-l", "m", "--vocab", "v", "--from-fasta", "--per-record"])
    assert a.per_record and not hasattr(a, "min_record_length")
    a = cli.parse_args(["image", "in", "--from-fasta"])
    assert not hasattr(a, "per_record") and not hasattr(a, "min_record_length")
