"""The read screen on the GPU (vk_screen_build_device, vk_screen_device, ImageEngine.screen_set / screen) against
tests/screen_ref.py: the set of every reference of tests/screen_cases.py key for key; text, lengths, the four stats and
the status of every case in both modes, with the match kernel's tile at SC.TILE bases in one engine and at its default in
another; a random case; the empty set; framing statuses; the error codes."""
import functools
import os
import random

import numpy as np
import pytest

import screen_cases as SC
import screen_ref as R
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc_engines():
    """"small" | "default" -> an ImageEngine whose context was made with VKIMG_SCREEN_TILE = SC.TILE (and units of 256
    bytes in the build) or with neither set."""
    from varkoder_amd.engine import ImageEngine
    cache = {}
    names = ("VKIMG_SCREEN_TILE", "VKIMG_FASTA_UNIT_BYTES")

    def get(tile):
        if tile not in cache:
            old = {n: os.environ.pop(n, None) for n in names}
            try:
                if tile == "small":
                    os.environ["VKIMG_SCREEN_TILE"] = str(SC.TILE)
                    os.environ["VKIMG_FASTA_UNIT_BYTES"] = "256"
                cache[tile] = ImageEngine(k=7, mapping="cgr", device=0)
            finally:
                for n in names:
                    os.environ.pop(n, None)
                    if old[n] is not None:
                        os.environ[n] = old[n]
        return cache[tile]
    yield get
    for e in cache.values():
        e.close()


def build(eng, fasta, k, slots=None):
    dev, _, _ = eng.upload([fasta])
    return eng.screen_set(dev, len(fasta), k, slots=slots)


def run(eng, sset, samples, keep, min_hits=1, records=None):
    """-> (each sample's text, out_lens, stats, status); the padding checked."""
    dev, offs, lens = eng.upload(samples)
    out, ooffs, olens, stats, status = eng.screen(dev, offs, lens, sset, keep=keep, min_hits=min_hits, records=records)
    host = out.cpu().numpy()
    assert all(int(o) % 16 == 0 for o in ooffs)
    for o, n in zip(ooffs, olens):   # zeros up to the 16-byte rounded end
        assert not host[int(o) + int(n):(int(o) + int(n) + 15) // 16 * 16].any()
    return [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(ooffs, olens)], olens, stats, status


@functools.lru_cache(maxsize=None)
def want_set(name):
    c = SC.BY_NAME[name]
    return R.set_ints(c.fasta, c.k), R.windows_ints(c.fasta, c.k)


@functools.lru_cache(maxsize=None)
def want_screen(name, keep):
    c = SC.BY_NAME[name]
    keys, _ = want_set(name)
    return [R.screen(text, keys, c.k, c.min_hits, keep) for text in c.samples]


@pytest.mark.parametrize("tile", ("small", "default"))
def test_the_set_of_every_reference(sc_engines, tile):
    """distinct count, table size and membership -- every key -- against the rule"""
    eng = sc_engines(tile)
    for c in SC.ALL_CASES:
        keys, windows = want_set(c.name)
        s = build(eng, c.fasta, c.k)
        assert (s.k, s.windows, s.distinct, s.slots) == (c.k, windows, len(keys), R.slots_for(windows)), c.name
        assert s.keys().tolist() == sorted(keys), c.name
    # 1,000 distinct keys in 1,024 slots: the same set
    c = SC.BY_NAME["ref_1000_keys"]
    s = build(eng, c.fasta, c.k, slots=1024)
    assert s.slots == 1024 and s.distinct == 1000 and s.keys().tolist() == sorted(want_set(c.name)[0])
    for keep in (False, True):
        got, _, _, _ = run(eng, s, c.samples, keep)
        assert got == [w[0] for w in want_screen(c.name, keep)]


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("tile", ("small", "default"))
def test_every_case_in_both_modes(sc_engines, tile, keep):
    eng = sc_engines(tile)
    for c in SC.ALL_CASES:
        s = build(eng, c.fasta, c.k)
        got, olens, stats, status = run(eng, s, c.samples, keep, c.min_hits)
        want = want_screen(c.name, keep)
        assert not status.any(), c.name
        assert got == [w[0] for w in want], c.name
        assert olens.tolist() == [len(w[0]) for w in want], c.name
        assert stats.tolist() == [w[1] for w in want], c.name


@pytest.mark.parametrize("k", (21, 31))
def test_random_reads_against_a_random_reference(sc_engines, k):
    """2,000 reads of 150 bases against 5,386 random bases; a tenth of the reads cut from it, on either strand, with 0 or 1
    substitution"""
    rng = random.Random(k)
    ref = SC.seq(rng, 5386)
    reads = []
    for i in range(2000):
        if i % 10 == 3:
            at = rng.randrange(len(ref) - 150)
            r = bytearray(ref[at:at + 150])
            if rng.random() < 0.5:
                p = rng.randrange(150)
                r[p] = rng.choice([b for b in b"ACGT" if b != r[p]])
            r = bytes(r)
            reads.append(SC.rc(r) if rng.random() < 0.5 else r)
        else:
            reads.append(SC.seq(rng, 150))
    fasta, text = SC.fa([(b"phix", ref)], 70), SC.fq(reads)
    keys = R.set_ints(fasta, k)
    eng = sc_engines("default")
    s = build(eng, fasta, k)
    assert s.distinct == len(keys) and s.keys().tolist() == sorted(keys)
    for keep in (False, True):
        for min_hits in (1, 40):
            want = R.screen(text, keys, k, min_hits, keep)
            got, olens, stats, status = run(eng, s, [text], keep, min_hits, records=[2000])
            assert status.tolist() == [0] and got == [want[0]] and stats.tolist() == [want[1]]
    assert R.screen(text, keys, k, 1, True)[1][1] == 200   # (every planted read and no other)


def test_the_empty_set_gives_the_input_back(sc_engines):
    eng = sc_engines("default")
    c = SC.BY_NAME["empty_set"]
    s = build(eng, c.fasta, c.k)
    assert s.distinct == 0 and s.slots == 1024
    got, olens, stats, status = run(eng, s, c.samples, False)
    assert got == list(c.samples) and not status.any()
    assert stats[:, 0].tolist() == stats[:, 1].tolist() and stats[:, 2].tolist() == stats[:, 3].tolist()
    got, olens, stats, _ = run(eng, s, c.samples, True)
    assert got == [b""] * len(c.samples) and not olens.any() and not stats[:, 1].any() and not stats[:, 3].any()


def test_a_sample_with_a_status_gets_no_text(sc_engines):
    eng = sc_engines("small")
    c = SC.BY_NAME["three_samples"]
    s = build(eng, c.fasta, c.k)
    good = c.samples[0]
    samples = [good, good[1:], good + b"@x\nACGT\n", good.replace(b"\n+\n", b"\n-\n", 1), good]
    want = [R.screen(t, want_set(c.name)[0], c.k, 1, False) for t in samples]
    assert [w[2] for w in want] == [0, R.VK_ST_BAD_START, R.VK_ST_BAD_PHASE, R.VK_ST_BAD_START, 0]
    got, olens, stats, status = run(eng, s, samples, False)
    assert status.tolist() == [w[2] for w in want]
    assert got == [w[0] for w in want] and stats.tolist() == [w[1] for w in want]
    # a record count that is not the sample's
    _, _, stats, status = run(eng, s, [good, good], False, records=[4, 3])
    assert status.tolist() == [0, _capi.VK_EM_BAD_RECORDS] and stats[1].tolist() == [0, 0, 0, 0]
    # a reference that does not begin with '>'
    with pytest.raises(ValueError):
        build(eng, b"ACGT" * 10 + b"\n", 21)


def test_error_codes(sc_engines):
    eng = sc_engines("default")
    c = SC.BY_NAME["three_samples"]
    s = build(eng, c.fasta, c.k)
    dev, offs, lens = eng.upload(list(c.samples))
    with pytest.raises(_capi.VkError) as e:   # a misaligned offset: before anything is read
        eng.screen(dev, [0, int(offs[1]) + 1, int(offs[2])], [int(lens[0]), int(lens[1]) - 1, int(lens[2])], s, records=[4, 3, 5])
    assert e.value.status == _capi.VK_EINVAL
    with pytest.raises(ValueError):
        eng.screen(dev, offs, lens, s, min_hits=0)
    for k in (15, 32):
        with pytest.raises(ValueError):
            build(eng, c.fasta, k)
    with pytest.raises(_capi.VkError) as e:   # a table that is no power of two
        build(eng, c.fasta, c.k, slots=1000)
    assert e.value.status == _capi.VK_EINVAL
    with pytest.raises(_capi.VkError) as e:   # 2,000 keys do not fit 1,024 slots
        build(eng, SC.fa([(b"r", SC.seq(random.Random(1), 2020))]), 21, slots=1024)
    assert e.value.status == _capi.VK_ENOSPC
    with pytest.raises(ValueError):           # more than 2^30 bytes of reference: refused before anything is allocated
        eng.screen_set(dev, (1 << 30) + 1, 21)
