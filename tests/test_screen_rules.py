"""tests/screen_ref.py states the rule of `--exclude-fasta` / `--keep-fasta` twice (strings; rolling integers): the two
agree on every case of tests/screen_cases.py, and the cases say what their names promise.  No GPU needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_cases as SC  # noqa: E402
import screen_ref as R  # noqa: E402


@pytest.mark.parametrize("case", SC.ALL_CASES, ids=lambda c: c.name)
def test_the_two_statements_agree(case):
    strings, ints = R.set_strings(case.fasta, case.k), R.set_ints(case.fasta, case.k)
    assert {R.key_of(w) for w in strings} == ints
    assert R.distinct_strings(strings) == len(ints)
    for keep in (False, True):
        for text in case.samples:
            a = R.screen(text, strings, case.k, case.min_hits, keep, hits=R.hits_strings)
            b = R.screen(text, ints, case.k, case.min_hits, keep, hits=R.hits_ints)
            assert a == b
            assert a[2] == 0
    for text in case.samples:
        for _, seq in R.split_records(text)[1]:
            assert R.hits_strings(seq, strings, case.k) == R.hits_ints(seq, ints, case.k)


@pytest.mark.parametrize("case", SC.ALL_CASES, ids=lambda c: c.name)
def test_the_cases_say_what_they_should(case):
    ints = R.set_ints(case.fasta, case.k)
    assert len(case.expect) == len(case.samples)
    for text, want in zip(case.samples, case.expect):
        st, recs = R.split_records(text)
        assert st == 0 and len(recs) == len(want)
        got = [R.hits_ints(seq, ints, case.k) >= case.min_hits for _, seq in recs]
        assert got == want
        # either mode: the kept records byte for byte, in order; together the two modes give every record once
        ex, ex_stats, _ = R.screen(text, ints, case.k, case.min_hits, False)
        kp, kp_stats, _ = R.screen(text, ints, case.k, case.min_hits, True)
        assert ex == b"".join(raw for (raw, _), m in zip(recs, want) if not m)
        assert kp == b"".join(raw for (raw, _), m in zip(recs, want) if m)
        assert b"".join(raw for raw, _ in recs) == bytes(text)
        assert ex_stats[0] == kp_stats[0] == len(recs) and ex_stats[1] + kp_stats[1] == len(recs)
        assert ex_stats[2] == kp_stats[2] == ex_stats[3] + kp_stats[3] == sum(len(seq) for _, seq in recs)


def test_particular_cases():
    by = SC.BY_NAME
    k = 21
    # exactly n - 1 and n hit POSITIONS, one key at several of them
    for n in (1, 2, 3):
        c = by["min_hits_%d_one_key" % n]
        ints = R.set_ints(c.fasta, c.k)
        assert len(ints) == 1
        hits = [R.hits_ints(seq, ints, c.k) for _, seq in R.split_records(c.samples[0])[1]]
        assert hits == [n - 1, n]
        c = by["min_hits_%d_distinct_keys" % n]
        ints = R.set_ints(c.fasta, c.k)
        assert len(ints) == 3
        assert [R.hits_ints(seq, ints, c.k) for _, seq in R.split_records(c.samples[0])[1]] == [n - 1, n]
    # the tile cases: one window of the read, and only one, is in the set
    tiles = [c for c in SC.READ_CASES if c.name.startswith("tiles_window_at_")]
    assert len(tiles) >= 10
    step = SC.TILE - (k - 1)
    spots = sorted(int(c.name.rsplit("_", 1)[1]) for c in tiles)
    for t in (1, 2, 3):
        assert t * step - 1 in spots and t * step in spots   # the last window of a tile, the first of the next
    for c in tiles:
        ints = R.set_ints(c.fasta, c.k)
        seq = R.split_records(c.samples[0])[1][0][1]
        assert len(ints) == 1 and R.hits_ints(seq, ints, c.k) == 1
        assert 3 * step + k - 1 < len(seq) < 4 * step   # 3 tiles plus a few bases
    # palindromes: one key, equal to its own reverse complement
    for kk in (16, 30):
        strings = R.set_strings(by["palindrome_k%d" % kk].fasta, kk)
        assert len(strings) == 1 and R.revcomp(next(iter(strings))) == next(iter(strings))
    # empty sets, distinct counts, table sizes
    for name in ("empty_set", "ref_short_records", "ref_header_only", "ref_empty_text"):
        assert R.set_ints(by[name].fasta, by[name].k) == set()
    one = len(R.set_ints(SC.fa([(b"u", by["ref_repeat_100_records"].fasta.split(b"\n")[1])]), k))
    assert one == 20
    for name in ("ref_repeat_100_records", "ref_repeat_100_line"):
        assert len(R.set_ints(by[name].fasta, k)) == one and R.windows_ints(by[name].fasta, k) == 100 * one
    big = by["ref_1000_keys"]
    assert len(R.set_ints(big.fasta, k)) == R.windows_ints(big.fasta, k) == 1000
    assert R.slots_for(1000) == 2048 and R.slots_for(512) == 1024 and R.slots_for(0) == 1024 and R.slots_for(513) == 2048
    # the junction key exists in neither reference, and would exist in the joined one
    j = by["ref_junction"]
    a, b = j.fasta.split(b">")[1:]
    joined = b"".join(a.split(b"\n")[1:]) + b"".join(b.split(b"\n")[1:])
    assert len(R.set_ints(SC.fa([(b"j", joined)]), k)) == len(R.set_ints(j.fasta, k)) + k - 1


def test_framing_statuses():
    ints = set()
    assert R.screen(b"r0\nACGT\n+\nIIII\n", ints, 21)[2] == R.VK_ST_BAD_START
    assert R.screen(b"@r0\nACGT\n+\nIIII\n@r1\nACGT\n", ints, 21)[2] == R.VK_ST_BAD_PHASE
    assert R.screen(b"@r0\nACGT\nIIII\n+\n", ints, 21)[2] == R.VK_ST_BAD_START
    assert R.ref_status(b"ACGT\n") == R.VK_ST_BAD_START and R.ref_status(b"") == 0 and R.ref_status(b">a\nACGT\n") == 0
