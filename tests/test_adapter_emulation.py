"""The lane-local device code of adapters by sequence, run on the host (tests/emul/adapter_emul.cpp compiles the
product's csrc/vk_adapter.h) against tests/adapter_ref.py: cl_trim_seq on every read of adapter_cases.trim_sweep() and
on seeded random reads of the same kind, ad_key_ok over every key, vk_ad_hist_kernel and vk_ad_collect_kernel over the
groups of adapter_cases.detect_edges().  Byte work: equality everywhere.  The emulation's header says what it does not
cover (the kernels with barriers and the host code of vkimg.hip: the GPU tests run those)."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_cases as AC  # noqa: E402
import adapter_emul_lib as EM  # noqa: E402
import adapter_ref as A  # noqa: E402

SLICE = 8          # groups per emulated launch (a table is 4 MiB)


# ----------------------------------------------------------------- trimming ---

def test_trim_seq_on_the_sweep():
    b = AC.trim_sweep()
    bad = [(s, ad) for s, ad in b["cases"] if EM.trim_seq(s, ad) != A.trim_by_sequence_literal(s, ad)]
    assert not bad, (len(bad), bad[:3])


def random_cases(seed=8401, nadapters=110):
    """At least 20,000 (read, adapter) of the sweep's kind: adapters of every length 1..64, a third of them with
    non-ACGT bytes."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(nadapters):
        L = i % AC.MAX_ADAPTER + 1 if i < 2 * AC.MAX_ADAPTER else int(rng.integers(1, AC.MAX_ADAPTER + 1))
        ad = bytearray(A._rng_seq(rng, L))
        if i % 3 == 0:
            for j in rng.integers(0, L, int(rng.integers(1, 4))):
                ad[j] = b"Nn.R"[int(rng.integers(0, 4))]
        ad = bytes(ad)
        reads = AC._sweep_reads(rng, ad, 170)
        if i % 3 == 0:
            reads += AC._faced(rng, ad, [j for j, c in enumerate(ad) if c not in b"ACGT"])
        out += [(s, ad) for s in reads]
    return out


def test_trim_seq_on_random_reads():
    cases = random_cases()
    assert len(cases) >= 20000
    bad = [(s, ad) for s, ad in cases if EM.trim_seq(s, ad) != A.trim_by_sequence_literal(s, ad)]
    assert not bad, (len(bad), bad[:3])
    c = AC.census_of(cases[::7])
    assert min(c) * 10 >= sum(c), c


def test_trim_seq_refuses_what_the_table_cannot_hold():
    assert EM.trim_seq(b"ACGT" * 10, b"") == 0xFFFFFFFF and EM.trim_seq(b"ACGT" * 10, b"A" * 65) == 0xFFFFFFFF


# -------------------------------------------------------------- key filters ---

def test_key_ok_over_every_key():
    got, want = EM.key_ok(), A.key_ok()
    assert got.shape == want.shape == (4 ** A.SEED_K,)
    assert (got == want).all(), np.flatnonzero(got != want)[:10]
    assert want[AC.key_of(AC.SEED)]


# ------------------------------------------------- histogram and occurrences ---

def edge_groups():
    """[(name, reads)] of detect_edges() without the large groups and the groups without records, plus reads of 29,
    30 and 31 bases (no window, one, two) around the seed."""
    d = AC.detect_edges()
    by_sample = {j: name for name, j in d["names"].items()}
    out = [(by_sample[j], d["reads"][j]) for j in AC.active_groups(d) if j not in d["large"]]
    P = d["P"]
    out.append(("len_29_30_31", [P[1:] + AC.SEED, P + AC.SEED, P + AC.SEED + b"T", (P + AC.SEED)[:29] + b"N"] * 20))
    assert {f"first_{sb}_{k}" for sb in (1, 10) for k in ("p19", "short_tail", "long_tail")} <= {n for n, _ in out}
    return out


def slices():
    g = edge_groups()
    for i in range(0, len(g), SLICE):
        part = g[i:i + SLICE]
        text = b"".join(AC._text(name.encode(), reads) for name, reads in part)
        yield part, text, [len(reads) for _, reads in part]


@functools.lru_cache(maxsize=None)
def key_ok():
    return A.key_ok()


def counts_of(reads):
    """What adapter_ref.candidates counts before it ranks (its own lines)."""
    m, _ = A._matrix(reads)
    key, valid = A._windows(m)
    valid[:, :A.SEED_FROM] = False
    counts = np.bincount(key[valid], minlength=4 ** A.SEED_K)
    counts[~key_ok()] = 0
    return counts


def test_hist_kernel_counts_what_candidates_counts():
    seen = 0
    for part, text, group_n in slices():
        got = EM.hist(text, group_n)
        for (name, reads), row in zip(part, got):
            want = counts_of(reads)
            assert (row == want).all(), (name, np.flatnonzero(row != want)[:5])
            cands, total = A.candidates(reads)       # (and the counts above are the ones candidates ranks)
            assert total == int(want.sum()) and all(int(want[k]) == c for k, c in cands), name
            seen += 1
    assert seen > 25
    d = dict(edge_groups())
    k = AC.key_of(AC.SEED)
    assert counts_of(d["first_1_p19"])[k] == A.MIN_VOTES - 1 and counts_of(d["first_1_all"])[k] == A.MIN_VOTES
    assert counts_of(d["len_29_30_31"])[k] == 40                  # the reads of 30 and 31 bases; none of 29


def occurrences(reads, key, T):
    """The occurrences that adapter_ref.extend takes for the seed, with their reaches: (read, p, forward, backward)."""
    m, lens = A._matrix(reads)
    keys, valid = A._windows(m)
    st = max(1, T)
    p = np.arange(keys.shape[1])[None, :]
    hit = valid & (keys == key) & (p >= A.SEED_FROM) & (p <= lens[:, None] - A.SEED_K - st)
    r, pp = np.nonzero(hit)
    return sorted((int(i), int(q), int(lens[i] - st - (q + A.SEED_K)), int(q)) for i, q in zip(r, pp))


@pytest.mark.parametrize("T", AC.TS)
def test_collect_kernel_lists_what_extend_takes(T):
    some = 0
    for part, text, group_n in slices():
        keys = np.zeros((len(part), EM.TOP), dtype=np.uint32)
        caps = np.zeros((len(part), EM.TOP), dtype=np.uint32)
        cands = [A.candidates(reads)[0] for _, reads in part]
        for k, cs in enumerate(cands):
            for c, (key, count) in enumerate(cs):
                keys[k, c], caps[k, c] = key, count
        counts, lists = EM.collect(text, group_n, keys, caps, max(1, T))
        nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
        seq_at = nl[0::4] + 1                                    # text offset of every record's first base
        first = np.concatenate([[0], np.cumsum(group_n)])
        for k, ((name, reads), cs) in enumerate(zip(part, cands)):
            for c in range(EM.TOP):
                if c >= len(cs):
                    assert counts[k, c] == 0 and lists[k][c] == [], name
                    continue
                want = occurrences(reads, cs[c][0], T)
                assert counts[k, c] == len(want) <= caps[k, c], (name, c)
                got = sorted(lists[k][c])
                assert got == sorted((int(seq_at[first[k] + r]) + p, f, bk) for r, p, f, bk in want), (name, c)
                assert (A.extend(reads, cs[c][0], T) is None) == (len(want) < A.MIN_VOTES), (name, c)
                some += len(want)
    assert some > 1000


# ---------------------------------------------------------------- sanitizers ---

def test_the_emulation_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program (its own main, never loaded into python) built with the sanitizers runs the sweep's reads
    through cl_trim_seq once: no byte read past a read or an adapter, no shift out of range, the same answers."""
    exe = EM.sanitizer_program(str(tmp_path))
    cases = AC.trim_sweep()["cases"]
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for s, ad in cases:
            f.write(struct.pack("<II", len(s), len(ad)) + s + ad)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = np.fromfile(dst, dtype="<u4")
    assert got.tolist() == [A.trim_by_sequence(s, ad) for s, ad in cases]
