"""tests/ladder_emit_ref.py, the rule of step C's files, pinned on the independent oracle (oracle/vk_oracle.c): the
text a step emits counts to what the oracle counts for the step, and holds the bases the oracle says it takes."""
import numpy as np
import pytest

import ladder_emit_ref as R
from oracle import oracle

KS = (5, 6, 7, 8, 9)


@pytest.fixture(scope="module")
def inputs():
    return {k: R.case_inputs(k) for k in KS}


def test_sample_hash_is_the_oracles():
    """thresholds h and h + 1 around the hash: the oracle takes the one read exactly from h + 1 on"""
    text = b"@r\nACGTACGTAC\n+\nIIIIIIIIII\n"
    for seed in (0, 7, (1 << 40) + 3):
        h = R.sample_hash(seed, 2)
        assert oracle.count_fastq_sampled(text, 5, seed, h)[3][1] == 0
        assert oracle.count_fastq_sampled(text, 5, seed, h + 1)[3][1] == 10


@pytest.mark.parametrize("k", KS)
def test_sampled_steps_count_to_the_oracles_sampled_count(inputs, k):
    for name, text in inputs[k].items():
        assert R.framing_status(text) == 0, name
        for seed in R.SEEDS:
            for thr in R.THRESHOLDS:
                out = R.emit_ref(text, seed, thr, whole=False)
                want, _, st, sites = oracle.count_fastq_sampled(text, k, seed, thr)
                got, _, st2 = oracle.count_fastq(out, k)
                assert st == 0 and st2 == 0, (name, seed, thr)
                assert np.array_equal(got, want), (name, seed, thr)
                # the oracle's sites are the bytes of the sequence lines, a '\r' among them; the files drop it: one byte
                # per read taken of a CRLF text, none anywhere else
                dropped = 0
                if name.startswith("crlf"):
                    dropped = sum(1 for a, _, _, _ in R.records(text) if R.sample_hash(seed, a) < thr)
                assert R.emitted_bases(out) + dropped == sites[1], (name, seed, thr)


@pytest.mark.parametrize("k", KS)
def test_whole_steps_count_to_the_plain_count(inputs, k):
    for name, text in inputs[k].items():
        out = R.emit_ref(text, 3, 0, whole=True)
        want, _, st = oracle.count_fastq(text, k)
        got, _, st2 = oracle.count_fastq(out, k)
        assert st == 0 and st2 == 0, name
        assert np.array_equal(got, want), name
        assert out.count(b"\n") == 4 * len(R.records(text)), name


def test_the_lines_of_a_record():
    text = b"@a x\r\nACNRacgt\r\n+a x\r\nIIIIIII!\r\n@b\n\n+\n\n@c\nAC\n+\nI#"
    assert R.emit_ref(text, 0, 1 << 32) == b"@a x\nACNNacgt\n+\nIIIIIII!\n@b\n\n+\n\n@c\nAC\n+\nI#\n"
    assert R.emit_ref(text, 0, 0) == b""
    long = b"@h\n" + b"A" * 1001 + b"\n+\n" + b"I" * 600 + b"\n"
    assert R.emit_ref(long, 0, 1 << 32) == (b"@h_1\n" + b"A" * 500 + b"\n+\n" + b"I" * 500 + b"\n@h_2\n" + b"A" * 500 +
                                            b"\n+\n" + b"I" * 100 + b"\n@h_3\nA\n+\n\n")
    assert R.emit_ref(long, 0, 1 << 32, whole=True) == long


def test_bad_framing_writes_nothing():
    for bad in (b"r\nAC\n+\nII\n", b"@r\nAC\nII\n", b"@r\nAC\n+\nII\n@s\nAC\n", b">r\nACGT\n"):
        assert R.framing_status(bad) and R.emit_ref(bad, 0, 1 << 32, whole=True) == b""
    assert R.framing_status(b"") == 0 and R.emit_ref(b"", 0, 1 << 32) == b""
