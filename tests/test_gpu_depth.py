"""The depth filter on the GPU (vk_depth_device, ImageEngine.spectrum(depth=...) and ImageEngine.depth_filter) against
tests/depth_ref.py, bit for bit -- output bytes, lengths, rows and status: every case of tests/depth_cases.py with the
kernels' tile at DC.TILE bases in one engine and at its default in another; the table forced to 1,024 slots at 900 and at
1,100 distinct keys; both ways of adding to the LDS histogram; three random samples in one group, in two and a group per
sample; the sample that overflows its first table; the error codes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import depth_cases as DC
import depth_ref as D
import spectrum_cases as SC
import spectrum_ref as R
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu

ENV = ("VKIMG_SPECTRUM_TILE", "VKIMG_DEPTH_MERGE")


@pytest.fixture(scope="module")
def dp_engines():
    """(tile, merge) -> an ImageEngine whose context was made with VKIMG_SPECTRUM_TILE = tile and VKIMG_DEPTH_MERGE = merge
    (None: not set)."""
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


def by_rule(samples, k, every, bands, slots=None):
    """(texts, lengths, rows, status) of one call by the rule."""
    got = [D.depth_count(t, k, every, lo, hi, slots) for t, (lo, hi) in zip(samples, bands)]
    return [g[0] for g in got], [len(g[0]) for g in got], [g[1].tolist() for g in got], [g[2] for g in got]


@functools.lru_cache(maxsize=None)
def want(name, every, bi):
    """A case's call by the rule: computed once, left unchanged."""
    c = DC.BY_NAME[name]
    return by_rule(c.samples, c.k, every, c.bandsets[bi], c.slots)


def run(eng, samples, k, every, bands, **kw):
    dev, offs, lens = eng.upload(list(samples))
    rows, status, out, ooffs, olens, drows, got_bands = eng.spectrum(dev, offs, lens, k=k, every=every, depth=list(bands), **kw)
    n = len(samples)
    assert drows.dtype == np.uint64 and drows.shape == (n, _capi.VK_DEPTH_NSTAT) and olens.dtype == np.uint64
    assert [b[:3] for b in got_bands] == [(lo, hi, True) for lo, hi in bands]
    assert all(int(o) % 16 == 0 for o in ooffs)
    host = out.cpu().numpy()
    texts = [host[int(o):int(o) + int(m)].tobytes() for o, m in zip(ooffs, olens)]
    for o, m in zip(ooffs, olens):   # (zeros up to the 16-byte rounded end)
        assert not host[int(o) + int(m):(int(o) + int(m) + 15) // 16 * 16].any()
    return (texts, [int(m) for m in olens], drows.tolist(), status.tolist()), rows.tolist()


@pytest.mark.parametrize("tile", (DC.TILE, None))
def test_every_case_equals_the_rule(dp_engines, tile):
    eng = dp_engines(tile)
    for c in DC.ALL_CASES:
        for every in c.everys:
            for bi, bands in enumerate(c.bandsets):
                got, _ = run(eng, c.samples, c.k, every, bands)
                assert got == want(c.name, every, bi), (c.name, every, bands)


def test_the_spectrum_describes_the_text_before_the_filter(dp_engines):
    eng = dp_engines()
    c = DC.BY_NAME["random_every_k21"]
    _, rows = run(eng, c.samples, c.k, 2, c.bandsets[1])
    assert rows == [R.spectrum_numpy(t, c.k, 2)[0].tolist() for t in c.samples]
    dev, offs, lens = eng.upload(list(c.samples))
    assert len(eng.spectrum(dev, offs, lens, k=c.k)) == 2   # (without a band: as ever)


@pytest.mark.parametrize("tile", (DC.TILE, None))
def test_a_table_forced_to_1024_slots(dp_engines, tile):
    """900 distinct keys: long probe chains and wrap-around, exact; 1,100: VK_SPEC_TABLE_FULL, no text and a zero row, the
    neighbours in the same call exact"""
    eng = dp_engines(tile)
    for c in DC.FORCED_CASES:
        for bi, bands in enumerate(c.bandsets):
            got, _ = run(eng, c.samples, c.k, 1, bands, slots=c.slots)
            assert got == want(c.name, 1, bi), (c.name, bands)
    texts, lens, rows, status = got
    assert status == [0, _capi.VK_SPEC_TABLE_FULL, 0] and lens[1] == 0 and not any(rows[1]) and rows[0][D.IN] == 2


def test_both_ways_of_adding_to_the_histogram(dp_engines):
    """VKIMG_DEPTH_MERGE = 0, 1: every taken lane adds, or a wave instruction on one bin adds once -- the same output"""
    names = [n % k for k in DC.KS for n in ("all_lanes_on_one_bin_k%d", "above_the_histogram_k%d", "tile_seam_k%d",
                                            "random_every_k%d", "median_at_the_edges_k%d")]
    for merge in (0, 1):
        for tile in (DC.TILE, None):
            eng = dp_engines(tile, merge)
            for name in names:
                c = DC.BY_NAME[name]
                for every in c.everys:
                    for bi, bands in enumerate(c.bandsets):
                        got, _ = run(eng, c.samples, c.k, every, bands)
                        assert got == want(name, every, bi), (name, every, bands, merge, tile)


@functools.lru_cache(maxsize=None)
def random_call():
    samples = SC.random_samples()
    return samples, by_rule(samples, 21, 1, DC.RANDOM_BANDS)


def test_three_random_samples_in_one_group_in_two_and_one_each(dp_engines):
    """three samples of 20,000 reads x 150 bases from 50 kb genomes at 1 % errors, one a quarter poly-A, a band each"""
    eng = dp_engines()
    samples, ref = random_call()
    assert all(0 < r[D.KEPT] < r[D.IN] for r in ref[2])   # (every band keeps some and drops some)
    assert ref[2][2][D.HIST_AT + 255] >= 5000             # (poly-A: above the histogram)
    one, _ = run(eng, samples, 21, 1, DC.RANDOM_BANDS, records=[20000] * 3)
    assert one == ref
    slots = [R.slots_for(len(t)) for t in samples]
    two, _ = run(eng, samples, 21, 1, DC.RANDOM_BANDS, table_bytes=12 * slots[0] * 2 + 1000)
    assert two == ref
    each, _ = run(eng, samples, 21, 1, DC.RANDOM_BANDS, table_bytes=1000)   # (smaller than any table: a group per sample)
    assert each == ref


def test_a_sample_counted_again_is_filtered_from_the_attempt_that_succeeded(dp_engines):
    eng = dp_engines()
    text = SC.overflow_sample()
    small = SC.BY_NAME["random_every_k16"].samples[0]
    samples, bands = [small, text, small], [(0, 0), (1, 1), (0, D.OPEN)]
    first = R.slots_for(len(text), 64)
    got, rows = run(eng, samples, 16, 64, bands)
    assert got == by_rule(samples, 16, 64, bands)
    assert got[3] == [0, 0, 0] and rows[1][R.DISTINCT] == 3000 > first and got[0][1] == text
    # the first table alone: full, no text, the neighbour exact
    got, _ = run(eng, samples[:2], 16, 64, bands[:2], slots=first)
    ref = by_rule(samples[:2], 16, 64, bands[:2], first)
    assert got == ref and got[3] == [0, _capi.VK_SPEC_TABLE_FULL] and got[1][1] == 0


def empty_tables(eng, n, slots=1024):
    import torch
    keys = torch.full((n * slots,), -1, dtype=torch.int64, device=eng.device)
    counts = torch.zeros(n * slots, dtype=torch.int32, device=eng.device)
    status = torch.zeros(n, dtype=torch.int32, device=eng.device)
    return keys, counts, np.arange(n, dtype=np.uint64) * np.uint64(slots), np.full(n, slots, dtype=np.uint64), status


def test_error_codes(dp_engines):
    import torch
    eng = dp_engines()
    c = DC.BY_NAME["random_every_k21"]
    text = c.samples[0]
    nrec = len(text.splitlines()) // 4
    dev, offs, lens = eng.upload([text])
    keys, counts, base, nsl, tstatus = empty_tables(eng, 1)
    cap = (int(lens[0]) + 15) // 16 * 16
    out = torch.full((cap + 16,), 0x5A, dtype=torch.uint8, device=eng.device)

    def call(**kw):
        a = dict(text=dev, offs=offs, lens=lens, keys=keys, counts=counts, base=base, nslots=nsl, table_status=tstatus,
                 lo=[0], hi=[0], k=21, every=1, records=[nrec], out=out, out_offs=[0])
        a.update(kw)
        return eng.depth_filter(**a)

    def einval(**kw):
        with pytest.raises(_capi.VkError) as e:
            call(**kw)
        assert e.value.status == _capi.VK_EINVAL, kw

    einval(lo=[3], hi=[2])
    einval(k=15)
    einval(k=32)
    einval(every=0)
    einval(nslots=np.array([1000], dtype=np.uint64))
    einval(offs=[int(offs[0]) + 1], lens=[int(lens[0]) - 1])            # a misaligned offset
    einval(out_offs=[8])
    einval(out=out[:cap - 16])                                            # an output capacity too small
    einval(out=out[:cap], out_offs=[16])
    assert bool((out == 0x5A).all())                                      # (nothing was written)
    # a null pointer
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))   # noqa: E731
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))   # noqa: E731
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=eng.device)
    d = torch.empty(512, dtype=torch.int64, device=eng.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    args = [eng.ctx, ptr(dev), u64(offs), u64(lens), u64([nrec]), 1, 21, 1, ptr(keys), ptr(counts), u64(base), u64(nsl),
            ptr(tstatus), u32([0]), u32([0]), ptr(out), u64([0]), int(out.numel()), ptr(d), ptr(d[8:]), ptr(d[300:]), ptr(ws),
            ws.numel()]
    for i in (1, 8, 9, 12, 13, 14, 15, 18, 19, 20, 21):
        bad = list(args)
        bad[i] = None
        assert eng.L.vk_depth_device(*bad) == _capi.VK_EINVAL, i
    assert eng.L.vk_depth_workspace_size(u64([nrec]), 1, u64(lens), None) == _capi.VK_EINVAL
    assert bool((out == 0x5A).all())
    # a record count that is not the sample's: no text, a zero row
    olens, rows, status = call(records=[nrec - 1])
    assert status.tolist() == [_capi.VK_EM_BAD_RECORDS] and olens.tolist() == [0] and not rows.any()
    # the spectrum's status joins the framing's
    olens, rows, status = call(table_status=torch.full((1,), _capi.VK_SPEC_TABLE_FULL, dtype=torch.int32, device=eng.device))
    assert status.tolist() == [_capi.VK_SPEC_TABLE_FULL] and olens.tolist() == [0] and not rows.any()
    # a key the table does not hold has depth 0: against empty tables 0:0 keeps every record, byte for byte
    olens, rows, status = call()
    assert status.tolist() == [0] and olens.tolist() == [len(text)] and out[:len(text)].cpu().numpy().tobytes() == text
    assert rows[0, D.IN] == rows[0, D.KEPT] == nrec == rows[0, D.HIST_AT]
    olens, rows, status = call(lo=[1], hi=[D.OPEN])
    assert olens.tolist() == [0] and rows[0, D.KEPT] == 0 and rows[0, D.IN] == nrec
    # explicit bands through spectrum(): lo above hi is the call's error, a band per sample is asked for
    with pytest.raises(_capi.VkError) as e:
        eng.spectrum(dev, offs, lens, depth=(3, 2))
    assert e.value.status == _capi.VK_EINVAL
    with pytest.raises(ValueError):
        eng.spectrum(dev, offs, lens, depth=[(0, 1), (0, 1)])
    got = eng.spectrum(dev, offs[:0], lens[:0], depth=(0, 1))
    assert len(got) == 7 and got[5].shape == (0, _capi.VK_DEPTH_NSTAT) and got[6] == []
