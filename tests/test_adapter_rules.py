"""Adapters by sequence in step B on the CPU: tests/adapter_ref.py's trimming at every boundary, detection on seeded
single-end sets, the key filters and the fold threshold, the listed adapters of the host and device code, and the
`image` flags that turn it on."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_ref as A  # noqa: E402

from varkoder_amd import adapters, cli  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


def rnd(seed, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, n)])


def trim(seq, ad):
    got = A.trim_by_sequence(seq, ad)
    assert got == A.trim_by_sequence_literal(seq, ad), (seq, ad)
    return got


# ----------------------------------------------------------------- trimming ---

@pytest.mark.parametrize("alen,start", [(7, 0), (8, -2), (12, -3), (16, -4), (33, -4)])
def test_start_buckets(alen, start):
    ad = rnd(alen, alen)
    body = rnd(100 + alen, 40)
    assert A.trim_start(alen) == start
    # the read starts with the adapter missing its first -start bases: cut at pos = start, emptied
    assert trim(ad[-start:] + body, ad) == 0
    # one base more missing: no negative offset reaches it
    assert trim(ad[-start + 1:] + body, ad) > 0
    # the adapter after 30 bases of insert
    assert trim(body[:30] + ad + body, ad) == 30


@pytest.mark.parametrize("alen,allowed", [(8, 1), (16, 2)])
def test_mismatch_limit(alen, allowed):
    ad = rnd(7 * alen, alen)
    ins = rnd(5, 30)
    for k, cut in ((allowed, True), (allowed + 1, False)):
        bad = bytearray(ad)
        for i in range(k):   # mismatches spread over the compared bases
            j = 1 + i * (alen - 2) // max(1, k)
            bad[j] = ord("A") if bad[j] != ord("A") else ord("C")
        got = trim(ins + bytes(bad) + b"T" * 20, ad)
        assert (got == 30) == cut, (k, got)


def test_last_four_bases():
    ad = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    ins = rnd(9, 60)
    assert trim(ins + ad[:5], ad) == 60          # pos = rlen - 5: compared (5 bases, no mismatch allowed)
    assert trim(ins + ad[:4], ad) == 64          # pos = rlen - 4: never tried
    assert trim(b"ACG", ad) == 3 and trim(b"", ad) == 0


def test_n_on_either_side():
    ad = b"CTGTCTCTTATACACATCT"                  # 19 bases: 2 mismatches allowed over 19
    ins = rnd(11, 30)
    tail = rnd(12, 10)
    n3 = bytearray(ad)
    for j in (2, 8, 14):
        n3[j] = ord("N")
    assert trim(ins + bytes(n3[:2]) + ad[2:] + tail, ad) == 30                 # no N: exact
    assert trim(ins + bytes(n3) + tail, ad) != 30                             # three N in the read: 3 mismatches
    assert trim(ins + bytes(n3[:9]) + ad[9:] + tail, ad) == 30                # two
    # an N in the adapter against an N in the read is equal bytes; against a base it is a mismatch
    assert trim(ins + bytes(n3) + tail, bytes(n3)) == 30
    assert trim(ins + ad + tail, bytes(n3)) != 30


def test_negative_pos_empties_the_read():
    ad = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    assert trim(ad[3:] + rnd(2, 50), ad) == 0    # adapter dimer without its first 3 bases (the A-tail skip)
    assert trim(ad + rnd(3, 50), ad) == 0


def test_literal_and_vectorised_agree():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        ad = rnd(int(rng.integers(1 << 30)), int(rng.integers(4, 40)))
        s = bytearray(rnd(int(rng.integers(1 << 30)), int(rng.integers(0, 60))) + ad[:int(rng.integers(0, len(ad) + 1))])
        for i in np.flatnonzero(rng.random(len(s)) < 0.05):
            s[i] = ord("N")
        trim(bytes(s), ad)


def test_clean_sample_adapters_without_adapters_is_clean_sample():
    r1, r2, se = A.R.synth_set(3, 400, 300)
    text, st, ad = A.clean_sample_adapters(r1, r2, se)
    assert (text, st) == A.R.clean_sample(r1, r2, se) and ad == dict(reads=0, bases=0)


def test_clean_sample_adapters_order():
    """Single reads: after poly-G; pairs: only when the overlap did not cut them; -a: nothing."""
    se = [(b"@s", rnd(1, 40) + A.TRUSEQ1 + b"G" * 30, b"I" * 103)]
    text, st, ad = A.clean_sample_adapters([], [], se, F=0, T=0, adapters=(None, None, A.TRUSEQ1))
    # (poly-G first: it takes the G tail and, within its mismatch budget, the adapter's last bases)
    assert text.split(b"\n")[1] == se[0][1][:40] and ad == dict(reads=1, bases=A.R.poly_g(se[0][1]) - 40)
    _, _, ad = A.clean_sample_adapters([], [], se, F=0, T=0, adapter=False, adapters=(None, None, A.TRUSEQ1))
    assert ad == dict(reads=0, bases=0)
    r1, r2 = A.pairs_with_adapters(4, 300, 0.5)
    _, _, ad = A.clean_sample_adapters(r1, r2, [], adapters=(A.TRUSEQ1, A.TRUSEQ2, None))
    assert ad["reads"] > 0


# ---------------------------------------------------------------- detection ---

def reads(recs):
    return [s for _, s, _ in recs]


@pytest.mark.parametrize("frac,want", [(0.05, A.TRUSEQ1), (0.3, A.TRUSEQ1), (0.0, None)])
def test_truseq_readthrough(frac, want):
    assert A.detect_adapter(reads(A.se_readthrough(1, 20000, frac))) == want


def test_nextera():
    assert A.detect_adapter(reads(A.se_readthrough(2, 20000, 0.2, adapter=A.NEXTERA))) == A.NEXTERA


def test_unlisted_dimers_accepted_unsnapped():
    got = A.detect_adapter(reads(A.dimers(3, 20000, 0.1)))
    assert got is not None and adapters.snap(got) is None
    assert A.UNLISTED[:20] in got and len(got) == A.MAX_DETECTED


def test_unlisted_readthrough_rejected():
    rs = reads(A.se_readthrough(4, 20000, 0.2, adapter=A.UNLISTED))
    cands, _ = A.candidates(rs)
    D, back_out, fwd_out = A.extend(rs, cands[0][0], 10)
    assert A.UNLISTED[10:26] in D and not back_out and fwd_out    # the backward extension breaks in the inserts
    assert A.detect_adapter(rs) is None


def test_genomic_repeat_rejected():
    rs = reads(A.repeat_reads(5, 20000, 0.2))
    assert len(A.candidates(rs)[0]) == A.TOP
    assert A.detect_adapter(rs) is None


def ok_keys(n):
    ok = A.key_ok()
    ks = np.flatnonzero(ok)[::7][:n]
    assert len(ks) == n
    return ks


@pytest.mark.parametrize("n,found", [(49932, True), (49933, False)])
def test_fold_threshold(n, found):
    """Reads of 30 bases hold one counted window (p = 20); n distinct keys once each: 4^10 // n is 21 or 20."""
    rs = [rnd(0, 20) + A.key_str(int(k)) for k in ok_keys(n)]
    cands, total = A.candidates(rs)
    assert total == n
    assert len(cands) == (A.TOP if found else 0)
    if found:   # ties in count: lexicographic order
        assert [k for k, _ in cands] == sorted(k for k, _ in cands)


@pytest.mark.parametrize("key,ok", [(b"AAAAAAAAAA", False), (b"AAAAAACGTC", False), (b"AAAAACGTCT", True),
                                    (b"GCGCGCGCAT", False), (b"GCGCGCGAAT", True), (b"GGGGACTACT", False),
                                    (b"GGGAGCTACT", True), (b"TTTTTTACGA", False), (b"ACGTACGTAC", True)])
def test_key_filters(key, ok):
    k = sum(b"ACGT".index(c) << (2 * (9 - i)) for i, c in enumerate(key))
    assert bool(A.key_ok()[k]) == ok
    # a set made of that key alone (plus noise) counts it only when it passes
    rs = [rnd(i, 20) + key + rnd(i + 7, 10) for i in range(300)]
    cands, total = A.candidates(rs)
    assert (cands[0][0] == k) == ok if cands else not ok


def test_evaluation_set_is_the_first_records():
    rs = reads(A.se_readthrough(6, 1000, 0.0)) * 300            # 300000 reads: the adapter only past 262144
    late = reads(A.se_readthrough(7, 30000, 0.5))
    assert A.detect_adapter(rs[:A.EVAL_RECORDS] + late) is None
    assert A.detect_adapter(late) == A.TRUSEQ1


# ------------------------------------------------------------ table and CLI ---

def test_device_table_equals_python_table():
    text = (ROOT / "varkoder_amd" / "csrc" / "vk_adapter.h").read_text()
    body = text[text.index("kAdKnown[]"):]
    body = body[:body.index("};")]
    assert tuple(re.findall(r'"([ACGT]+)"', body)) == tuple(s.decode() for _, s in adapters.KNOWN_ADAPTERS)
    assert f"kAdSnap = {adapters.SNAP_BASES};" in text


def test_snap_first_in_table_order():
    assert adapters.snap(b"TT" + A.TRUSEQ1[:16] + b"CC") == A.TRUSEQ1
    assert adapters.snap(A.TRUSEQ1[:15]) is None
    assert adapters.snap(b"AGATCGGAAGAGCGTCGTGT") == A.TRUSEQ2
    assert adapters.snap(A.NEXTERA[:16]) == A.NEXTERA and adapters.snap(A.NEXTERA[1:]) is None


def test_new_flags_parse():
    a = cli.parse_args(["image", "in", "--from-raw", "--detect-adapters", "--adapter-sequence", "acgtacgtac",
                        "--adapter-sequence-r2", "TTTTCCCC"])
    assert a.detect_adapters is True and a.adapter_sequence == b"ACGTACGTAC" and a.adapter_sequence_r2 == b"TTTTCCCC"
    a = cli.parse_args(["image", "in", "--from-raw"])
    for name in ("detect_adapters", "adapter_sequence", "adapter_sequence_r2"):
        assert not hasattr(a, name)


@pytest.mark.parametrize("argv", [["image", "in", "--detect-adapters"],
                                  ["image", "in", "--from-clean", "--adapter-sequence", "ACGTACGT"],
                                  ["image", "in", "--from-raw", "-a", "--detect-adapters"],
                                  ["image", "in", "--from-raw", "-a", "--adapter-sequence-r2", "ACGT"],
                                  ["image", "in", "--from-raw", "--adapter-sequence", "ACG"],
                                  ["image", "in", "--from-raw", "--adapter-sequence", "ACGTN"],
                                  ["image", "in", "--from-raw", "--adapter-sequence", "A" * 65]])
def test_refusals(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    assert "adapter" in capsys.readouterr().err


def test_no_short_flags():
    p = cli.setup_parser()
    image = p._subparsers._group_actions[0].choices["image"]
    for act in image._actions:
        if act.dest in ("detect_adapters", "adapter_sequence", "adapter_sequence_r2"):
            assert all(o.startswith("--") for o in act.option_strings)
