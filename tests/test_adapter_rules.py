"""Adapters by sequence in step B on the CPU: tests/adapter_ref.py's trimming at every boundary, detection on seeded
single-end sets, the key filters and the fold threshold, the listed adapters of the host and device code, and the
`image` flags that turn it on.  Then the reference on tests/adapter_cases.py's batches, which the emulation and the GPU
tests run as well: it gives every planted result, and the batches hold what they are said to hold."""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_cases as AC  # noqa: E402
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


# ------------------------------------------------- adapter_cases: trim_sweep ---

def test_sweep_census_and_shape():
    b = AC.trim_sweep()
    assert [len(t[2]) for t in b["adapters"][:AC.MAX_ADAPTER]] == list(range(1, AC.MAX_ADAPTER + 1))
    assert set(b["dirty"]) == set(AC.ASSERTED) and len(b["pairs"]) >= 8
    assert all(l1 != l2 for _, l1, l2 in b["pairs"])
    uncut, emptied, between = b["census"]
    n = len(b["cases"])
    assert uncut + emptied + between == n and n > 200 * AC.MAX_ADAPTER
    assert min(uncut, emptied, between) * 10 >= n, b["census"]
    lens = {len(s) for s, _ in b["cases"]}
    assert set(range(6)) <= lens and max(lens) > 150


@pytest.mark.parametrize("L", AC.ASSERTED)
def test_sweep_sample_by_sample(L):
    """The clean and the dirty sample of an adapter length: the expected stats are the literal rule's, read by read;
    every class of the census occurs; a negative offset empties reads that do not start with the adapter's start."""
    b = AC.trim_sweep()
    want = AC.sweep_expected()
    for j in (L - 1, b["dirty"][L]):
        ad = b["adapters"][j][2]
        assert len(ad) == L
        _, _, se, status = AC.K.groups(b)[j]
        reads = bases = 0
        classes = set()
        shifted = 0
        for rec in se:
            s = A.R._trim(rec, 0, 0)[1]
            n = trim(s, ad)
            reads += n < len(s)
            bases += len(s) - n
            classes.add(0 if n == len(s) else 1 if n == 0 else 2)
            shifted += n == 0 and len(s) > 4 and s[:1] != ad[:1] and L >= 8
        assert status == 0 and want[j][3] == [reads, bases] and reads > 20
        assert classes == {0, 1, 2} and (shifted > 0) == (A.trim_start(L) < 0)
        assert want[j][0].count(b"\n") // 4 == want[j][1][1] < len(se)           # emptied reads are not written


def test_sweep_pairs_keep_one_mate():
    b = AC.trim_sweep()
    want = AC.sweep_expected()
    for j, l1, l2 in b["pairs"]:
        r1, r2, _, _ = AC.K.groups(b)[j]
        a1, a2, _ = b["adapters"][j]
        assert (len(a1), len(a2)) == (l1, l2)
        only = [0, 0]
        for x, y in zip(r1, r2):
            sx, sy = A.R._trim(x, 0, 0)[1], A.R._trim(y, 0, 0)[1]
            assert A.R.overlap(sx, sy) is None or A.R.overlap(sx, sy)[0] >= 0      # the overlap cuts none of them
            nx, ny = trim(sx, a1), trim(sy, a2)
            only[0] += nx == 0 and ny > 0
            only[1] += ny == 0 and nx > 0
        assert min(only) >= 3, (j, only)
        assert want[j][3][0] > 60


# ----------------------------------------------- adapter_cases: detect_edges ---

def small_groups(d):
    return [(name, j) for name, j in d["names"].items() if j not in d["large"]]


@pytest.mark.parametrize("T", AC.TS)
def test_edges_reference_gives_the_planted_result(T):
    d = AC.detect_edges()
    planted = 0
    for name, j in small_groups(d):
        want = d["planted"][T][j]
        got = A.detect_adapter(d["reads"][j], T)
        if want is not AC.FREE:
            assert got == want, (name, T, got, want)
            planted += 1
        assert A.group_adapters([], [], [(b"", s, b"") for s in d["reads"][j]], T=T) == [None, None, got]
    assert planted >= 20


def test_edges_side_conditions():
    d = AC.detect_edges()
    names, reads, planted = d["names"], d["reads"], d["planted"]
    U, P = d["U"], d["P"]
    assert A.key_ok()[AC.key_of(AC.SEED)]
    # votes, consensus, reach
    assert planted[10][names["votes_at"]] == U[:60] and planted[10][names["votes_under"]] is None
    assert reads[names["votes_at"]].count(U[:70]) == A.MIN_VOTES == reads[names["votes_under"]].count(U[:70]) + 1
    cands, _ = A.candidates(reads[names["consensus_under"]])
    assert len(cands) == A.TOP and all(c == 100 for _, c in cands)
    stopped = 0
    for key, _ in cands:     # every ranked seed stops at the changed base: one direction does not run out
        ext = A.extend(reads[names["consensus_under"]], key, 10)
        if ext is not None:  # (None: the seed lies where T = 10 lets no extension start)
            assert not (ext[1] and ext[2]) and (ext[0].startswith(U[46:56]) or ext[0].endswith(U[35:45]))
            stopped += 1
    assert stopped >= 3
    assert [planted[T][names["reach"]] for T in AC.TS] == [U[:60], U[:60], U[:60], U[:45]]
    # the first counted position: the odd read's seed at p = 19, its tail one short, one long
    for sb, g in d["first_position"].items():
        full, odd = reads[g["all"]][0], {k: reads[g[k]][-1] for k in ("p19", "short_tail", "long_tail")}
        assert full.find(AC.SEED) == A.SEED_FROM and len(full) == A.SEED_FROM + A.SEED_K + sb
        assert odd["p19"].find(AC.SEED) == A.SEED_FROM - 1 and len(odd["p19"]) == len(full)
        assert len(odd["short_tail"]) == len(full) - 1 and len(odd["long_tail"]) == len(full) + 1
        for T in AC.TS:
            if max(1, T) == sb:
                assert [planted[T][g[k]] for k in ("all", "p19", "short_tail", "long_tail")] == [P + AC.SEED, None, None, P + AC.SEED]
    # snapping
    for (name, nx), j in d["snap"].items():
        ad = A.TRUSEQ1 if name == "truseq1" else AC.NEXTERA
        D = reads[j][0][:A.MAX_DETECTED]
        assert planted[10][j] == (ad if nx == 44 else D) and (adapters.snap(D) == ad) == (nx == 44)
    # the ring wraps; the forward cap is passed
    for name, p, forward in (("ring", 70, False), ("cap", A.SEED_FROM, True)):
        rs = reads[names[name]]
        for T in AC.TS:
            key = A.candidates(rs)[0][0][0]
            assert rs[0].find(A.key_str(key), A.SEED_FROM) == p and rs[0].count(A.key_str(key)) == 1
            m, lens = A._matrix(rs)
            occ_r, occ_p = np.arange(len(rs)), np.full(len(rs), p)
            steps, out = A._extend(m, lens, occ_r, occ_p, forward, max(1, T))
            assert out and len(steps) == (len(rs[0]) - max(1, T) - p - A.SEED_K if forward else p) > 64
            assert A.extend(rs, key, T) == (rs[0][:A.MAX_DETECTED], True, True)
    # N in the consensus
    for T in AC.TS:
        D = planted[T][names["with_n"]]
        assert D[15:16] == b"N" and D[50:51] == b"N"
    # ties, and more than one slice of groups with no-candidate groups on both sides of the boundary
    assert len(reads[names["ties"]]) == 49932 and len(A.candidates(reads[names["ties"]])[0]) == A.TOP
    active = AC.active_groups(d)
    assert len(active) > 32 and names["zero_records"] not in active and names["no_files"] not in active
    assert names["no_files"] not in d["owner"]
    none = [i for i, j in enumerate(active) if j not in d["large"] and not A.candidates(reads[j])[0]]
    assert any(i < 32 for i in none) and any(i >= 32 for i in none)
    assert all(planted[T][active[i]] is None for i in none for T in AC.TS)
    assert A.candidates(reads[names["poly"]])[1] == 0 and max(map(len, reads[names["short"]])) < 30


_CANDS = {}


def detect_large(reads, T):
    """adapter_ref.detect_adapter on a large set with what does not depend on T done once: the candidates of the
    whole set, and of its reads only those that hold a candidate's 10-mer (extend looks at no other read)."""
    if id(reads) not in _CANDS:
        cands, total = A.candidates(reads)
        kmers = [A.key_str(k) for k, _ in cands]
        _CANDS[id(reads)] = cands, total, [s for s in reads if any(k in s for k in kmers)]
    cands, _, holding = _CANDS[id(reads)]
    for key, _ in cands:
        ext = A.extend(holding, key, T)
        if ext is None:
            continue
        D, back_out, fwd_out = ext
        s = adapters.snap(D)
        if s is not None:
            return s
        if back_out and fwd_out:
            return D
    return None


@pytest.mark.parametrize("name,T", [("fold_at", 0), ("fold_over", 0), ("eval_at", 10), ("eval_under", 10)])
def test_edges_large_groups(name, T):
    """The whole reference once at the T the group was made for; detect_large, held equal to it there, at the others."""
    d = AC.detect_edges()
    j = d["names"][name]
    reads = d["reads"][j]
    assert j in d["large"] and len(reads) <= A.EVAL_RECORDS
    assert A.detect_adapter(reads, T) == d["planted"][T][j] == detect_large(reads, T)
    for t in AC.TS:
        assert detect_large(reads, t) == d["planted"][t][j] is not AC.FREE, (name, t)
    total = _CANDS[id(reads)][1]
    if name.startswith("fold"):
        at = A.MIN_VOTES * 4 ** A.SEED_K // (A.FOLD + 1)
        assert total == (at if name == "fold_at" else at + 1) and reads.count(d["P"] + AC.SEED + b"G") == A.MIN_VOTES
        assert A.MIN_VOTES * 4 ** A.SEED_K // total == (A.FOLD + 1 if name == "fold_at" else A.FOLD)
        assert d["planted"][0][j] == (d["P"] + AC.SEED if name == "fold_at" else None)
    else:
        n = A.MIN_VOTES if name == "eval_at" else A.MIN_VOTES - 1
        files = [i for i, o in enumerate(d["owner"]) if o == j]
        assert len(files) == 2 and d["records"][files[0]] == 200000 and len(reads) == A.EVAL_RECORDS
        assert sum(d["records"][i] for i in files) == A.EVAL_RECORDS - n + 100
        assert reads.count(d["U"][:70]) == n and reads[-n:] == [d["U"][:70]] * n
        assert d["planted"][10][j] == (d["U"][:60] if name == "eval_at" else None)
        # a budget that ends as many dimers into file 2, well below the evaluation set's size
        rec, breads, bplanted = AC.budget_records(d)
        assert sum(rec[i] for i in files) == len(breads[j]) < A.EVAL_RECORDS - 90000
        assert breads[j].count(d["U"][:70]) == n and bplanted[j] == d["planted"][10][j]
        assert detect_large(breads[j], 10) == bplanted[j]


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
