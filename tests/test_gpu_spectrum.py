"""The k-mer spectrum on the GPU (vk_spectrum_device, ImageEngine.spectrum) against tests/spectrum_ref.py, bit for bit,
rows and status: every case of tests/spectrum_cases.py with the count kernel's tile at SC.TILE bases in one engine and at
its default in another; the table forced to 1,024 slots at 900 and at 1,100 distinct keys; the resize path of every > 1;
a random call of three samples in one group and in two; every way the count kernel merges equal keys; the error codes."""
import functools
import os

import numpy as np
import pytest

import spectrum_cases as SC
import spectrum_ref as R
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu

ENV = ("VKIMG_SPECTRUM_TILE", "VKIMG_SPECTRUM_MERGE")


@pytest.fixture(scope="module")
def sp_engines():
    """(tile, merge) -> an ImageEngine whose context was made with VKIMG_SPECTRUM_TILE = tile and VKIMG_SPECTRUM_MERGE =
    merge (None: not set)."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(tile=None, merge=None):
        if (tile, merge) not in cache:
            old = {n: os.environ.pop(n, None) for n in ENV}
            try:
                for n, v in zip(ENV, (tile, merge)):
                    if v is not None:
                        os.environ[n] = str(v)
                cache[(tile, merge)] = ImageEngine(k=7, mapping="cgr", device=0)
            finally:
                for n in ENV:
                    os.environ.pop(n, None)
                    if old[n] is not None:
                        os.environ[n] = old[n]
        return cache[(tile, merge)]
    yield get
    for e in cache.values():
        e.close()


@functools.lru_cache(maxsize=None)
def want(name, every):
    """(rows, status) of a case by the rule: computed once, left unchanged."""
    c = SC.BY_NAME[name]
    got = [R.spectrum_numpy(t, c.k, every, c.slots) for t in c.samples]
    return [r.tolist() for r, _ in got], [s for _, s in got]


def run(eng, samples, k, every=1, **kw):
    dev, offs, lens = eng.upload(list(samples))
    rows, status = eng.spectrum(dev, offs, lens, k=k, every=every, **kw)
    assert rows.dtype == np.uint64 and rows.shape == (len(samples), _capi.VK_SPEC_NSTAT) and status.dtype == np.uint32
    return rows.tolist(), status.tolist()


@pytest.mark.parametrize("tile", (SC.TILE, None))
def test_every_case_equals_the_rule(sp_engines, tile):
    eng = sp_engines(tile)
    for c in SC.ALL_CASES:
        for every in c.everys:
            assert run(eng, c.samples, c.k, every) == want(c.name, every), (c.name, every)


@pytest.mark.parametrize("tile", (SC.TILE, None))
def test_a_table_forced_to_1024_slots(sp_engines, tile):
    """900 distinct keys: long probe chains and wrap-around, exact; 1,100: VK_SPEC_TABLE_FULL and a zero row, the
    neighbours in the same call exact"""
    eng = sp_engines(tile)
    for c in SC.FORCED_CASES:
        rows, status = run(eng, c.samples, c.k, 1, slots=c.slots)
        assert (rows, status) == want(c.name, 1), c.name
    assert status == [0, _capi.VK_SPEC_TABLE_FULL, 0] and not any(rows[1]) and rows[0][R.DISTINCT] > 0


def test_every_way_of_merging_equal_keys(sp_engines):
    """VKIMG_SPECTRUM_MERGE = 0, 1, 2: none, runs in neighbouring lanes, the wave's table -- the same rows"""
    names = [n % k for k in SC.KS for n in ("poly_a_600_k%d", "bin_edges_k%d", "tile_seam_k%d", "random_every_k%d", "palindrome_16_k%d")]
    for merge in (0, 1, 2):
        for tile in (SC.TILE, None):
            eng = sp_engines(tile, merge)
            for name in names:
                c = SC.BY_NAME[name]
                for every in c.everys:
                    assert run(eng, c.samples, c.k, every) == want(name, every), (name, every, merge, tile)


def test_a_table_that_fills_at_every_above_1_is_counted_again(sp_engines):
    eng = sp_engines()
    text = SC.overflow_sample()
    small = SC.BY_NAME["random_every_k16"].samples[0]
    first = R.slots_for(len(text), 64)
    # the first table alone: full, the neighbour exact
    rows, status = run(eng, [small, text], 16, 64, slots=first)
    assert status == [0, _capi.VK_SPEC_TABLE_FULL] and not any(rows[1])
    assert rows[0] == R.spectrum_numpy(small, 16, 64)[0].tolist()
    # the engine's own sizes: four times the slots the second time
    rows, status = run(eng, [small, text, small], 16, 64)
    assert status == [0, 0, 0]
    assert rows == [R.spectrum_numpy(t, 16, 64)[0].tolist() for t in (small, text, small)]
    assert rows[1][R.DISTINCT] == 3000 > first


def test_three_random_samples_in_one_group_and_in_two(sp_engines):
    """three samples of 20,000 reads x 150 bases from 50 kb genomes at 1 % errors, one a quarter poly-A"""
    eng = sp_engines()
    samples = SC.random_samples()
    ref = [R.spectrum_numpy(t, 21)[0].tolist() for t in samples]
    rows, status = run(eng, samples, 21, records=[20000] * 3)
    assert status == [0, 0, 0] and rows == ref
    assert rows[2][R.HIST_AT + 255] >= 1   # (poly-A: in the overflow bin)
    # table_bytes below the three tables, above two of them: two groups
    slots = [R.slots_for(len(t)) for t in samples]
    assert len(set(slots)) == 1
    split, _ = run(eng, samples, 21, table_bytes=12 * slots[0] * 2 + 1000)
    assert split == ref
    one_each, _ = run(eng, samples, 21, table_bytes=1000)   # (smaller than any table: a group per sample)
    assert one_each == ref
    sampled, _ = run(eng, samples[2:], 21, every=16)
    assert sampled == [R.spectrum_numpy(samples[2], 21, 16)[0].tolist()]


def test_error_codes(sp_engines):
    eng = sp_engines()
    c = SC.BY_NAME["random_every_k21"]
    dev, offs, lens = eng.upload(list(c.samples))
    for k in (15, 32):
        with pytest.raises(ValueError):
            eng.spectrum(dev, offs, lens, k=k)
    with pytest.raises(ValueError):
        eng.spectrum(dev, offs, lens, every=0)
    for slots in (1000, 512):   # no power of two; below 1,024
        with pytest.raises(_capi.VkError) as e:
            eng.spectrum(dev, offs, lens, slots=slots)
        assert e.value.status == _capi.VK_EINVAL
    with pytest.raises(_capi.VkError) as e:   # a misaligned offset: before anything is read
        eng.spectrum(dev, [int(offs[0]) + 1], [int(lens[0]) - 1], records=[1])
    assert e.value.status == _capi.VK_EINVAL
    # a record count that is not the sample's
    rows, status = eng.spectrum(dev, offs, lens, records=[len(c.samples[0].splitlines()) // 4 - 1])
    assert status.tolist() == [_capi.VK_EM_BAD_RECORDS] and not rows.any()
    rows, status = eng.spectrum(dev, offs[:0], lens[:0])
    assert rows.shape == (0, _capi.VK_SPEC_NSTAT) and status.shape == (0,)
