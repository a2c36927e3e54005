"""The rule of `--qc-report` (tests/qc_ref.py) held to itself, and the host arithmetic of varkoder_amd/qc.py: the two
statements of the rule agree on every stream of every case of tests/qc_cases.py; the sums a row must satisfy; qc.add_rows,
qc.profile, qc.report and qc.columns on rows computed by hand; for a single-end sample the `after` content counts of cycles
0..39 are what tests/clean_ref.py counts for `<sample>_fastp_gpu.json` (rawinput.content_curves' rule).  No GPU."""
import functools
import json

import numpy as np
import pytest

import clean_ref as C
import qc_cases as QC
import qc_ref as R
from varkoder_amd import _capi, qc, rawinput


@functools.lru_cache(maxsize=None)
def cases():
    return QC.all_cases()


def test_the_constants_are_the_headers():
    assert (R.NSTAT, R.QUAL_AT, R.READQ_AT, R.LEN_AT, R.BASE_AT, R.QSUM_AT, R.CYCLES) == \
        (_capi.VK_QC_NSTAT, _capi.VK_QC_QUAL_HIST, _capi.VK_QC_READQ_HIST, _capi.VK_QC_LEN_HIST, _capi.VK_QC_CYCLE_BASE,
         _capi.VK_QC_CYCLE_QSUM, _capi.VK_QC_CYCLES)
    assert R.NSTAT == 8 + 94 + 94 + 1025 + 1024 * 5 + 1024 * 5
    assert (R.VK_QC_BAD_FRAMING, R.VK_EM_BAD_RECORDS) == (_capi.VK_QC_BAD_FRAMING, _capi.VK_EM_BAD_RECORDS)


@pytest.mark.parametrize("make", QC.CASES, ids=lambda m: m.__name__)
def test_the_two_statements_agree(make):
    case = make()
    for i, (text, n) in enumerate(case.streams):
        a, sa = R.row_loop(text, n)
        b, sb = R.row_numpy(text, n)
        assert sa == sb, (case.name, i)
        assert np.array_equal(a, b), (case.name, i, np.flatnonzero(a != b)[:8])


def test_the_cases_hold_what_they_are_named_for():
    by = {c.name: c for c in cases()}
    row, st = R.row(*by["length_sweep"].streams[0])
    assert st == 0 and int(row[R.RECORDS]) == len(QC.SWEEP_LENGTHS) and int(row[R.MAX_LEN]) == 20000 and int(row[R.MIN_LEN]) == 0
    assert int(row[R.LEN_AT + 1024]) == 6 and int(row[R.LEN_AT]) == 1   # 1024, 1025, 4095, 4096, 4097 and 20000 share the last bin
    status = [R.row(t, n)[1] for t, n in by["budgets"].streams]
    assert status == [0, 0, 0, 0, 8, 16, 16, 0, 16, 16, 0, 16, 16, 0, 8, 0]
    assert [int(R.row(t, n)[0][R.RECORDS]) for t, n in by["budgets"].streams[:4]] == [0, 1, 129, 130]
    framing = [R.row(t, n) for t, n in by["framing"].streams]
    assert all(st == 0 for _, st in framing)
    assert np.array_equal(framing[0][0], framing[1][0]) and np.array_equal(framing[0][0], framing[3][0])   # CRLF, no final \n
    assert np.array_equal(framing[0][0], framing[2][0]) and np.array_equal(framing[0][0], framing[4][0])   # +name
    assert int(framing[6][0][R.INVALID]) == 6 and int(framing[7][0][R.RAGGED]) == 4 and int(framing[7][0][R.RECORDS]) == 5
    assert int(framing[8][0][R.RAGGED]) == 1 and not framing[8][0][2:].any()
    row, _ = R.row(*by["carry"].streams[0])
    assert int(row[R.QSUM_AT + 0 * 5 + 0]) == 93 * 70000 and int(row[R.BASE_AT + 35 * 5 + 3]) == 70000


def test_the_sums_of_a_row():
    for case in cases():
        for text, n in case.streams:
            row, st = R.row(text, n)
            if st:
                assert not row.any()
                continue
            q = row[R.QUAL_AT:R.QUAL_AT + R.PHREDS]
            assert int(q.sum()) == int(row[R.BASES])
            ln = row[R.LEN_AT:R.LEN_AT + R.LEN_BINS]
            assert int(ln.sum()) == int(row[R.RECORDS]) - int(row[R.RAGGED])
            assert int(row[R.READQ_AT:R.READQ_AT + R.PHREDS].sum()) == int(ln[1:].sum())
            base = row[R.BASE_AT:R.BASE_AT + R.CYCLES * 5].reshape(R.CYCLES, 5)
            qsum = row[R.QSUM_AT:R.QSUM_AT + R.CYCLES * 5]
            if int(row[R.MAX_LEN]) < 1024:   # every base lies in the cycle tables
                assert int(base.sum()) == int(row[R.BASES])
                assert int(qsum.sum()) == int((q * np.arange(R.PHREDS, dtype=np.uint64)).sum())
                assert int(base[:, 1].sum() + base[:, 2].sum()) == int(row[R.GC]) and int(base[:, 4].sum()) == int(row[R.OTHER])
            # the reads that reach cycle c, from the length histogram
            reach = int(ln.sum()) - np.concatenate(([0], np.cumsum(ln[:-1]))).astype(np.int64)[1:]
            assert np.array_equal(base.sum(axis=1).astype(np.int64), reach)


def hand_row():
    """@a ACGTN / II5+! (40 40 20 10 0), @b GG / ?? (30 30), @c ragged."""
    return R.row(b"@a\nACGTN\n+\nII5+!\n@b\nGG\n+\n??\n@c\nAC\n+\nI\n", 3)[0]


def test_profile_and_report_by_hand():
    row = hand_row()
    p = qc.profile(row)
    assert (p["total_reads"], p["total_bases"], p["q20_bases"], p["q30_bases"]) == (3, 7, 5, 4)
    assert p["q20_rate"] == 5 / 7 and p["q30_rate"] == 4 / 7 and p["mean_length"] == 3.5 and p["gc_content"] == 4 / 7
    assert (p["total_cycles"], p["min_length"], p["max_length"], p["ragged_reads"], p["invalid_quality_bytes"]) == (5, 2, 5, 1, 0)
    assert p["content_curves"]["A"] == [0.5, 0.0, 0.0, 0.0, 0.0] and p["content_curves"]["G"] == [0.5, 0.5, 1.0, 0.0, 0.0]
    assert p["content_curves"]["N"] == [0.0, 0.0, 0.0, 0.0, 1.0] and p["content_curves"]["GC"] == [0.5, 1.0, 1.0, 0.0, 0.0]
    assert p["content_curves"]["T"] == [0.0, 0.0, 0.0, 1.0, 0.0] and p["content_curves"]["C"] == [0.0, 0.5, 0.0, 0.0, 0.0]
    assert p["quality_curves"]["A"] == [40.0, 0.0, 0.0, 0.0, 0.0] and p["quality_curves"]["G"] == [30.0, 30.0, 20.0, 0.0, 0.0]
    assert p["quality_curves"]["mean"] == [35.0, 35.0, 20.0, 10.0, 0.0]
    assert p["length_histogram"] == [0, 0, 1, 0, 0, 1]
    assert [i for i, v in enumerate(p["quality_histogram"]) if v] == [0, 10, 20, 30, 40] and sum(p["quality_histogram"]) == 7
    assert [(i, v) for i, v in enumerate(p["read_mean_quality_histogram"]) if v] == [(22, 1), (30, 1)]
    empty = qc.profile(R.zero_row())
    assert empty["q30_rate"] == 0.0 and empty["mean_length"] == 0.0 and empty["gc_content"] == 0.0 and empty["total_cycles"] == 0
    assert empty["length_histogram"] == [0] and empty["content_curves"]["A"] == []
    other = R.row(b"@d\nACGTACGTAC\n+\nIIIIIIIIII\n", 1)[0]
    both = qc.add_rows([row, other, R.zero_row()])
    assert (int(both[R.RECORDS]), int(both[R.BASES]), int(both[R.MIN_LEN]), int(both[R.MAX_LEN])) == (4, 17, 2, 10)
    assert np.array_equal(both[8:], row[8:] + other[8:])
    assert not qc.add_rows([]).any()
    rep = qc.report({"read1": row, "read2": other}, other)
    assert set(rep) == {"summary", "read1_before_filtering", "read2_before_filtering", "after_filtering"}
    assert rep["summary"]["before_filtering"] == qc.totals(both) and rep["summary"]["after_filtering"] == qc.totals(other)
    assert set(rep["summary"]["before_filtering"]) == {"total_reads", "total_bases", "q20_bases", "q30_bases", "q20_rate",
                                                       "q30_rate", "mean_length", "gc_content"}
    assert rep["read1_before_filtering"] == p and rep["after_filtering"] == qc.profile(other)
    only = qc.report(None, other)
    assert set(only) == {"summary", "after_filtering"} and set(only["summary"]) == {"after_filtering"}
    assert set(qc.report({"single": row}, other)) == {"summary", "single_before_filtering", "after_filtering"}
    json.dumps(rep)   # (plain numbers and lists)
    cols = qc.columns(both, other)
    assert list(cols) == ["raw_reads", "raw_basepairs", "raw_q30_rate", "clean_reads", "clean_q30_rate", "clean_gc_content",
                          "clean_mean_length"]
    assert cols == {"raw_reads": 4, "raw_basepairs": 17, "raw_q30_rate": 14 / 17, "clean_reads": 1, "clean_q30_rate": 1.0,
                    "clean_gc_content": 0.5, "clean_mean_length": 10.0}
    assert list(qc.columns(None, other)) == ["clean_reads", "clean_q30_rate", "clean_gc_content", "clean_mean_length"]
    assert not [c for c in cols if c.endswith("_time")]
    assert qc.report_path("d", "s").name == "s.qc.json" and "_fastp_" not in qc.report_path("d", "s").name


def test_after_content_counts_are_clean_refs_for_a_single_end_sample():
    _, _, singles = C.synth_set(91, 0, 1200)
    text, st = C.clean_sample([], [], singles)
    row, status = R.row(text, R.record_count(text))
    assert status == 0 and int(row[R.RECORDS]) == st["records"] and int(row[R.BASES]) == st["clean_bp"]
    base = row[R.BASE_AT:R.BASE_AT + 40 * 5].reshape(40, 5)
    assert np.array_equal(base[:, :4].astype(np.int64), np.array(st["base"]))
    assert np.array_equal(base.sum(axis=1).astype(np.int64), np.array(st["reach"]))
    want = rawinput.content_curves(np.array(st["base"]).ravel(), st["reach"])
    got = qc.profile(row)["content_curves"]
    assert all(got[b][:40] == want[b] for b in "ATCG")
