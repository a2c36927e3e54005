"""The BGZF compressor's member kernel (csrc/vk_deflate.h) compiled for the host (tests/emul/deflate_emul.cpp), its
lanes run one after another, over the texts of tests/deflate_cases.py with the assertions of the GPU test.  zlib is the
judge.  No GPU needed.

This covers the ARITHMETIC of vk_deflate.h only: barriers, LDS atomics, the gather kernel and the C entry points run in
tests/test_gpu_deflate.py alone.  What ties the two together is tests/golden/deflate_sweep_sha256.json: the digest of
the emulation's file for every text, checked here against the emulation and there against the GPU's bytes."""
import json
import os
import subprocess
import zlib

import pytest

import deflate_cases as D
import deflate_emul_lib as EM
import deflate_tokens as T

GUARD = EM.GUARD


@pytest.fixture(scope="module")
def emul():
    return EM.load()


def _run_all(emul, named):
    out = []
    for name, text in named:
        rc, data, guard = emul(text)
        assert rc == 0 and (guard == GUARD).all(), name
        out.append((name, text, data))
    return out


@pytest.fixture(scope="module")
def files(emul):
    return _run_all(emul, list(D.texts().items()) + [(f"small_{i}", t) for i, t in enumerate(D.small_files())])


@pytest.fixture(scope="module")
def sweep_files(emul):
    return _run_all(emul, list(D.sweep().items()))


def test_every_file_inflates_to_its_text_and_is_bgzf(files):
    from varkoder_amd import engine as E
    for name, text, data in files:
        D.check_file(name, text, data)
        assert E.bgzf_members(data) is not None and E.bgzf_text_size(data) == len(text), name


def test_a_second_run_gives_the_same_bytes(emul, files):
    for name, text, data in files[:40]:
        assert emul(text)[1] == data, name


def test_bound_and_a_buffer_one_byte_short(emul):
    assert [emul.bound(n) for n in (0, 1, 65280, 65281)] == [32, 64, 65344, 65376]
    for n in (0, 1, 65280, 65281, 200000):
        assert emul.bound(n) == (D.bound(n) + 15) // 16 * 16
    text = D.texts()["fastq_long_header"]
    rc, data, guard = emul(text, cap=emul.bound(len(text)) - 1)
    assert rc == 6 and data is None and (guard == GUARD).all()


def test_what_zlib_level_1_itself_does_with_the_size_checks():
    """The figures quoted in tests/test_gpu_deflate.py's docstring: level 1 meets both conditions on the FASTQ-shaped
    texts and the repeated record, and misses the first on the skewed text."""
    for name, text in D.texts().items():
        if not (name.startswith("fastq_") or name in ("skewed", "repeated")):
            continue
        for at in range(0, len(text), D.MEMBER):
            t = text[at:at + D.MEMBER]
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            size = len(c.compress(t) + c.flush()) + D.FRAMING
            ok = size <= D.huffman_only_size(t) + D.TABLE_ALLOWANCE + D.FRAMING
            assert ok == (name != "skewed"), (name, size, D.huffman_only_size(t))
            if name == "repeated":
                assert 2 * size < D.huffman_only_size(t)


# ---- the token reader, on zlib's own streams ----------------------------------------------------------------

def _zlib_raw(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(text) + c.flush()


def test_the_token_reader_on_streams_from_zlib():
    """deflate_tokens reads what zlib wrote: its own expansion of the tokens is zlib.decompress's text, the tokens' lengths
    add up to it, a copy never reaches before the text, and every symbol's code length is in the table it reports."""
    texts = D.texts()
    cases = [texts[k][:12000] for k in ("repeated", "skewed", "uniform256", "fastq_ragged", "random", "one_value")]
    cases += [texts["far"], D.sweep()["every_length"][:12000], D.sweep()["period_257"], b"abracadabra" * 40]
    seen, read = set(), 0
    for text in cases:
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY),
                                (6, zlib.Z_HUFFMAN_ONLY), (0, zlib.Z_DEFAULT_STRATEGY)):
            raw = _zlib_raw(text, level, strategy)
            try:
                blocks, mine, end = T.read_deflate(raw)
            except ValueError as e:   # (zlib takes the fixed code where that is smaller)
                assert "BTYPE 1" in str(e)
                continue
            read += 1
            assert mine == zlib.decompress(raw, -15) == text and end == len(raw)
            at = 0
            for b in blocks:
                seen.add(b.btype)
                assert b.btype in (0, 2) and (level != 0 or b.btype == 0)
                if b.btype == 2:
                    assert len(b.ll_lengths) == b.hlit + 257 and len(b.d_lengths) == b.hdist + 1 and b.ll_lengths[256]
                for tok in b.tokens:
                    assert tok[0] == at
                    if len(tok) == 2:
                        assert b.btype == 0 or b.ll_lengths[tok[1]]
                        at += 1
                    else:
                        assert strategy != zlib.Z_HUFFMAN_ONLY and 3 <= tok[1] <= 258 and 1 <= tok[2] <= min(at, 32768)
                        assert b.ll_lengths[T.length_symbol(tok[1])] and b.d_lengths[T.distance_symbol(tok[2])]
                        assert text[at:at + tok[1]] == (text[at - tok[2]:at] * (tok[1] // tok[2] + 1))[:tok[1]]
                        at += tok[1]
            assert at == len(text) and blocks[-1].final and not any(b.final for b in blocks[:-1])
    assert seen == {0, 2} and read >= 30
    # a member: header with an extra field and a name, one block, trailer
    import gzip
    import io
    buf = io.BytesIO()
    with gzip.GzipFile("name.fq", "wb", 6, buf, mtime=0) as g:
        g.write(texts["repeated"])
    block, mine = T.read_member(buf.getvalue())
    assert mine == texts["repeated"] and block.btype == 2 and any(len(t) == 3 for t in block.tokens)


def test_the_token_reader_refuses_what_it_does_not_read():
    """Fixed-Huffman blocks (Z_FIXED, and zlib's choice for short texts) are refused, not guessed at: the compressor
    writes none.  So are a cut stream, BTYPE 3 and a stored block whose two lengths disagree."""
    with pytest.raises(ValueError, match="BTYPE 1"):
        T.read_deflate(_zlib_raw(D.texts()["repeated"], 6, zlib.Z_FIXED))
    with pytest.raises(ValueError, match="BTYPE 1"):
        T.read_deflate(_zlib_raw(b"short", 6))
    raw = _zlib_raw(D.texts()["repeated"], 6)
    with pytest.raises(ValueError):
        T.read_deflate(raw[:len(raw) // 2])
    with pytest.raises(ValueError, match="BTYPE 3"):
        T.read_deflate(b"\x07\x00")
    with pytest.raises(ValueError, match="disagree"):
        T.read_deflate(b"\x01\x03\x00\xfc\xfe" + b"abc")
    assert [T.length_symbol(n) for n in (3, 10, 11, 12, 13, 257, 258)] == [257, 264, 265, 265, 266, 284, 285]
    assert [T.distance_symbol(d) for d in (1, 4, 5, 6, 7, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 28, 29, 29]


# ---- the sweep ------------------------------------------------------------------------------------------------------

def test_the_sweep_is_what_the_issue_lists():
    s = D.sweep()
    assert all(f"period_{p}" in s and len(s[f"period_{p}"]) == max(3000, 2 * p + 700) for p in D.PERIODS)
    assert all(f"dist_{d}" in s for d in D.DISTANCES) and len(D.DISTANCES) == 56 and D.DISTANCES[-1] == 32768
    assert all(len(s[f"len_{n}"]) == n and s[f"len_{n}"] == s["len_1100"][:n] for n in range(1, 1101))
    for name in ("two_symbols", "one_symbol_and_one", "all_256_flat"):
        assert len(s[name]) == D.MEMBER
    assert len(set(s["two_symbols"])) == 2 and len(set(s["one_symbol_and_one"])) == 2 and len(set(s["all_256_flat"])) == 256
    assert all(len(s[name]) <= D.MEMBER for name in ("skewed_with_matches", "skewed_distances", "every_length"))
    fuzz = [s[f"fuzz_{i}"] for i in range(D.FUZZ)]
    assert D.FUZZ == 300 and max(map(len, fuzz)) > 65280 and min(map(len, fuzz)) == 0 and max(map(len, fuzz)) <= 70_000
    assert s == D.sweep(), "seeded"


def test_every_sweep_file_inflates_to_its_text_and_a_second_run_gives_the_same_bytes(emul, sweep_files):
    """check_file, the guard bytes (in the fixture) and a second run, for every text of the sweep."""
    for name, text, data in sweep_files:
        D.check_file(name, text, data)
        rc, again, guard = emul(text)
        assert rc == 0 and again == data and (guard == GUARD).all(), name


def census(named_files):
    """What the compressor wrote for a list of (name, text, file): every member's block through the token reader."""
    c = {"length_symbols": set(), "distance_symbols": set(), "lengths": set(), "distances": set(), "stored": 0,
         "dynamic_without_match": 0, "dynamic_with_matches": 0, "ll_bits": 0, "d_bits": 0, "no_distance": 0, "one_distance": 0,
         "covering": 0, "member_length_mod_256": set(), "deepest": {}}
    for name, text, data in named_files:
        for member, mtext in D.members_of(data)[:-1]:
            block, mine = T.read_member(member)
            assert mine == mtext, name
            c["member_length_mod_256"].add(len(mtext) % 256)
            if block.btype == 0:
                c["stored"] += 1
                continue
            matches = [t for t in block.tokens if len(t) == 3]
            used = {T.distance_symbol(t[2]) for t in matches}
            c["dynamic_with_matches" if matches else "dynamic_without_match"] += 1
            c["length_symbols"] |= {T.length_symbol(t[1]) for t in matches}
            c["distance_symbols"] |= used
            c["lengths"] |= {t[1] for t in matches}
            c["distances"] |= {t[2] for t in matches}
            c["covering"] += sum(1 for t in matches if t[0] % 256 + t[1] >= 512)
            for key, table in (("ll_bits", block.ll_lengths), ("d_bits", block.d_lengths)):
                if max(table) > c[key]:
                    c[key] = max(table)
                    c["deepest"][key] = name
            if not used and block.hdist + 1 == 2:
                c["no_distance"] += 1
            if len(used) == 1:
                c["one_distance"] += 1
    return c


def test_census_of_the_tokens_that_the_lists_make_the_compressor_write(files, sweep_files):
    """The conditions that keep texts() + sweep() from testing nothing, read from the files with deflate_tokens.  A
    condition that fails is met by changing a generator in deflate_cases, never by relaxing it here.

    Both halves of the 15-bit condition hold: `skewed` and `skewed_with_matches` bring the literal/length code to its
    limit, `skewed_distances` the distance code (17 distance symbols used in proportions a little over Fibonacci's,
    about 5,500 matches in 44 KB)."""
    named = [f for f in files if not f[0].startswith("small_")] + sweep_files
    c = census(named)
    assert c["length_symbols"] == set(range(257, 286)), sorted(set(range(257, 286)) - c["length_symbols"])
    assert c["distance_symbols"] == set(range(30)), sorted(set(range(30)) - c["distance_symbols"])
    assert {257, 258} <= c["lengths"] and {1, 32768} <= c["distances"]
    assert set(range(3, 259)) <= c["lengths"], sorted(set(range(3, 259)) - c["lengths"])
    assert set(D.DISTANCES) <= c["distances"], sorted(set(D.DISTANCES) - c["distances"])
    assert c["stored"] >= 1 and c["dynamic_without_match"] >= 1 and c["dynamic_with_matches"] >= 200, c
    assert c["ll_bits"] == 15 and c["d_bits"] == 15, (c["ll_bits"], c["d_bits"])
    assert c["no_distance"] >= 1 and c["one_distance"] >= 1
    assert c["covering"] >= 1
    assert c["member_length_mod_256"] == set(range(256))
    # the named cases do what they are named for
    by = {name: data for name, _, data in sweep_files}

    def block(name):
        return T.read_member(D.members_of(by[name])[0][0])[0]
    b = block("skewed_with_matches")   # the tokens' block, and more symbols at 15 bits than an unlimited code has at its deepest
    assert sum(len(t) == 3 for t in b.tokens) > 5000 and max(b.ll_lengths) == 15 and b.ll_lengths.count(15) > 2
    b = block("skewed_distances")
    assert max(b.d_lengths) == 15 and b.d_lengths.count(15) > 2
    for at in (254, 255):
        assert (at, 258, 1) in block(f"covered_round_{at}").tokens
    assert any(t[0] == 1024 + 254 and t[1:] == (258, 1024 + 254) for t in block("covered_round_far").tokens)
    assert block("all_256_flat").btype == 0
    b = block("one_symbol_and_one")
    assert {t[2] for t in b.tokens if len(t) == 3} == {1} and [t[1] for t in b.tokens if len(t) == 2] == [ord("G"), ord("A")]
    for d in D.DISTANCES:
        assert any(len(t) == 3 and t[2] == d for t in block(f"dist_{d}").tokens), d


# ---- the recorded digests -------------------------------------------------------------------------------------------

def test_the_recorded_digests_are_the_emulations(files, sweep_files):
    """tests/golden/deflate_sweep_sha256.json is what the GPU's bytes are compared with (tests/test_gpu_deflate.py, on a
    machine that needs no compiler for it): it must be the emulation's output of today, entry by entry."""
    with open(D.DIGESTS) as f:
        recorded = json.load(f)
    assert recorded == D.digests(EM.compress, files + sweep_files)


def test_the_gather_batch_reaches_every_alignment():
    """The condition of the GPU's gather test, on the emulation's sizes (the GPU's are the same by the digest check): in
    the 40 files of 3..5 members every residue mod 4 of a member's offset in its file occurs in at least 8 non-first
    members."""
    texts = D.gather_files()
    assert len(texts) == 40 and all(3 <= -(-len(t) // D.MEMBER) <= 5 for t in texts) and 7e6 < sum(map(len, texts)) < 9e6
    residues = [0, 0, 0, 0]
    for t in texts:
        at = 0
        for i, (member, _) in enumerate(D.members_of(EM.compress(t))[:-1]):
            if i:
                residues[at % 4] += 1
            at += len(member)
    assert min(residues) >= 8, residues


def test_the_scan_batch_is_what_the_gpu_test_needs():
    texts = D.scan_files()
    D.check_scan_batch(texts)


# ---- sanitizers -----------------------------------------------------------------------------------------------------

def test_the_emulation_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program (its own main, never loaded into python) built with the sanitizers, once over the lists:
    texts(), 30 of the small files, the sweep's named families and 30 of its fuzz texts."""
    exe = EM.sanitizer_program(str(tmp_path))
    sweep = D.sweep()
    named = list(D.texts().items()) + [(f"small_{i}", t) for i, t in enumerate(D.small_files()[:30])]
    named += [(k, v) for k, v in sweep.items() if not k.startswith("fuzz_")]
    named += [(f"fuzz_{i}", sweep[f"fuzz_{i}"]) for i in range(0, D.FUZZ, 10)]
    paths = []
    for name, text in named:
        p = os.path.join(tmp_path, name)
        with open(p, "wb") as f:
            f.write(text)
        paths.append(p)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    for (name, text), p in zip(named, paths):
        with open(p + ".gz", "rb") as f:
            D.check_file(name, text, f.read())
