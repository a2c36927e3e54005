"""The sketches on the GPU (vk_sketch_device, vk_sketch_pairs_device; ImageEngine.spectrum(sketch=...), sketch_tables,
sketch_pairs) against tests/sketch_ref.py, bit for bit.  Through the spectrum: eligible at s - 1, s and s + 1;
multiplicities m - 1 and m at m = 1, 2, 3; a badly framed and a full-table sample beside good ones; three samples of
different table sizes in one group, one with more eligible keys than its buffer holds; the resize path of every > 1.  On
hand-made tables (tests/sketch_cases.py): tables of one and of two workgroups, hashes that share their top 11, 22, 33 and
44 bits, a crossing bin of one and of all, s of 64, s just above the run length, s = 2^20, a key in 7,000 slots; the error
codes.  Pairs: 9 x 31 and more, lengths 0, 1, s - 1 and s, identical, disjoint and interleaved sketches, a common value at
every segment seam, `q is r`; the error codes."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import screen_ref
import sketch_cases as KC
import sketch_ref as R
import spectrum_cases as SC
import spectrum_ref as SR
from screen_cases import fq, rc, seq
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu

ONES = np.uint64(R.MASK)


@pytest.fixture(scope="module")
def eng():
    from varkoder_amd.engine import ImageEngine
    e = ImageEngine(k=7, mapping="cgr", device=0)
    yield e
    e.close()


def want_sample(text, k, every, m, s, status=0):
    """(row of s hashes, [eligible, length]) of a sample by the rule, through the first statement of the spectrum's."""
    if status or screen_ref.split_records(text)[0]:
        return R.row([], s), [0, 0]
    counts = SR.counts_loop(text, k, every)[3]
    sk, eligible = R.sketch_np(list(counts.keys()), list(counts.values()), m, s)
    return R.row(sk, s), [eligible, len(sk)]


def run_spectrum(eng, samples, k, s, m, every=1, **kw):
    dev, offs, lens = eng.upload(list(samples))
    rows, status, hashes, info = eng.spectrum(dev, offs, lens, k=k, every=every, sketch=(s, m), **kw)
    plain = eng.spectrum(dev, offs, lens, k=k, every=every, **kw)
    assert np.array_equal(plain[0], rows) and np.array_equal(plain[1], status)   # (the rows do not know of the sketch)
    assert hashes.dtype == np.uint64 and hashes.shape == (len(samples), s) and info.shape == (len(samples), 2)
    return status.tolist(), hashes, info


def check_spectrum(eng, samples, k, s, m, every=1, **kw):
    status, hashes, info = run_spectrum(eng, samples, k, s, m, every, **kw)
    for i, t in enumerate(samples):
        row, inf = want_sample(t, k, every, m, s, status[i])
        assert info[i].tolist() == inf and np.array_equal(hashes[i], row), (i, inf, info[i].tolist())
    return status, info


def test_eligible_at_s_minus_1_s_and_s_plus_1(eng):
    rng = random.Random(11)
    s, k = 64, 21
    samples = [fq(SC.distinct_kmers(rng, n, k)) for n in (s - 1, s, s + 1)]
    status, info = check_spectrum(eng, samples, k, s, 1)
    assert status == [0, 0, 0] and info.tolist() == [[63, 63], [64, 64], [65, 64]]


@pytest.mark.parametrize("m", (1, 2, 3))
def test_multiplicities_m_minus_1_and_m(eng, m):
    rng = random.Random(20 + m)
    k = 21
    mers = SC.distinct_kmers(rng, 300, k)
    reads = []
    for i, x in enumerate(mers):   # a third of the keys m - 1 times (none at m = 1), a third m times, a third m + 1 times
        reads += [x if j % 2 else rc(x) for j in range(m - 1 + i % 3)]
    rng.shuffle(reads)
    status, info = check_spectrum(eng, [fq(reads)], k, 64, m)
    assert status == [0] and info.tolist() == [[200, 64]]


def test_bad_and_full_samples_beside_good_ones(eng):
    c = SC.BY_NAME["bad_framing_between_good_k21"]
    status, info = check_spectrum(eng, c.samples, c.k, 64, 1)
    assert [bool(x) for x in status] == [bool(screen_ref.split_records(t)[0]) for t in c.samples] and sum(map(bool, status)) >= 2
    assert info[1].tolist() == [0, 0] and info[0, 1] == 64
    c = SC.BY_NAME["forced_1024_slots_1100_keys"]
    status, info = check_spectrum(eng, c.samples, c.k, 64, 1, slots=c.slots)
    assert status == [0, _capi.VK_SPEC_TABLE_FULL, 0] and info[1].tolist() == [0, 0] and info[0, 0] > 0


def test_three_table_sizes_in_one_group(eng):
    """tables of 1,024, 8,192 and 65,536 slots; the last holds 20,000 keys, more than its buffer of 6,144: the select runs"""
    rng = random.Random(33)
    samples = [fq([seq(rng, 200)]), fq([seq(rng, 3000)]), fq([seq(rng, 20020)])]
    assert [SR.slots_for(len(t)) for t in samples] == [1024, 8192, 65536]
    for s, m in ((64, 1), (3000, 1)):
        status, info = check_spectrum(eng, samples, 21, s, m)
        assert status == [0, 0, 0] and info[2].tolist() == [20000, s]


def test_the_resize_path_of_every_above_1(eng):
    text = SC.overflow_sample()
    small = SC.BY_NAME["random_every_k16"].samples[0]
    status, info = check_spectrum(eng, [small, text, small], 16, 256, 1, every=64)
    assert status == [0, 0, 0] and info[1].tolist() == [3000, 256]
    # the first table alone: full, no sketch
    status, info = check_spectrum(eng, [small, text], 16, 256, 1, every=64, slots=SR.slots_for(len(text), 64))
    assert status == [0, _capi.VK_SPEC_TABLE_FULL] and info[1].tolist() == [0, 0]


# ---------------------------------------------------------- hand-made tables --

def run_tables(eng, tables, s, m, status=None):
    import torch
    nsl = np.array([len(t.keys) for t in tables], dtype=np.uint64)
    base = np.zeros(len(tables), dtype=np.uint64)
    base[1:] = np.cumsum(nsl[:-1])
    keys = torch.from_numpy(np.concatenate([t.keys for t in tables]).view(np.int64)).to(eng.device)
    counts = torch.from_numpy(np.concatenate([t.counts for t in tables]).view(np.int32)).to(eng.device)
    st = torch.tensor(status or [0] * len(tables), dtype=torch.int32, device=eng.device)
    return eng.sketch_tables(keys, counts, base, nsl, st, s, m)


@functools.lru_cache(maxsize=None)
def hand():
    return KC.hand_tables()


def test_hand_made_tables_one_call_each(eng):
    for t in hand():
        sk, eligible = R.sketch_np(t.keys, t.counts, t.m, t.s)
        hashes, info = run_tables(eng, [t], t.s, t.m)
        assert info.tolist() == [[eligible, len(sk)]] and np.array_equal(hashes[0], R.row(sk, t.s)), t.name


def test_hand_made_tables_in_one_call_and_a_status_between(eng):
    """all tables of s = 64 and m = 1 as the samples of one call, every third with a status: those are empty, the others exact"""
    tables = [t for t in hand() if t.s == 64 and t.m == 1]
    assert len(tables) >= 9
    status = [5 if i % 3 == 1 else 0 for i in range(len(tables))]
    hashes, info = run_tables(eng, tables, 64, 1, status)
    for i, t in enumerate(tables):
        sk, eligible = ([], 0) if status[i] else R.sketch_np(t.keys, t.counts, 1, 64)
        assert info[i].tolist() == [eligible, len(sk)] and np.array_equal(hashes[i], R.row(sk, 64)), t.name


def test_s_of_2_20_with_2000_eligible(eng):
    t = KC.big_table()
    sk, eligible = R.sketch_np(t.keys, t.counts, t.m, t.s)
    hashes, info = run_tables(eng, [t], t.s, t.m)
    assert info.tolist() == [[2000, 2000]] and np.array_equal(hashes[0, :2000], sk) and (hashes[0, 2000:] == ONES).all()


def test_a_key_in_7000_slots_is_bounded_and_counts_once_per_slot(eng):
    t = KC.duplicate_table()
    sk, eligible = R.sketch_np(t.keys, t.counts, t.m, t.s)
    hashes, info = run_tables(eng, [t], t.s, t.m)
    assert info.tolist() == [[eligible, t.s]] and np.array_equal(hashes[0], sk)


def test_sketch_error_codes(eng):
    import torch
    L = eng.L
    keys = torch.full((1024,), -1, dtype=torch.int64, device=eng.device)
    counts = torch.zeros(1024, dtype=torch.int32, device=eng.device)
    status = torch.zeros(1, dtype=torch.int32, device=eng.device)
    out = torch.zeros(64, dtype=torch.int64, device=eng.device)
    info = torch.zeros(2, dtype=torch.int64, device=eng.device)
    one = (C.c_uint64 * 1)
    base, nsl, b = one(0), one(1024), C.c_uint64()
    assert L.vk_sketch_workspace_size(nsl, 1, 64, C.byref(b)) == _capi.VK_OK and b.value > 0
    ws = torch.zeros(int(b.value), dtype=torch.uint8, device=eng.device)
    p = eng._ptr

    def call(ctx=eng.ctx, k=p(keys), c=p(counts), base=base, nsl=nsl, n=1, st=p(status), m=1, s=64, h=p(out), i=p(info), w=p(ws),
             wb=None):
        return L.vk_sketch_device(ctx, k, c, base, nsl, n, st, m, s, h, i, w, ws.numel() if wb is None else wb)
    assert call() == _capi.VK_OK
    assert eng.L.vk_ctx_sync(eng.ctx) == _capi.VK_OK
    assert info.tolist() == [0, 0] and (out == -1).all()
    for kw in (dict(ctx=None), dict(k=None), dict(c=None), dict(base=None), dict(nsl=None), dict(st=None), dict(h=None),
               dict(i=None), dict(w=None), dict(n=0), dict(m=0), dict(s=63), dict(s=(1 << 20) + 1), dict(wb=int(b.value) - 1),
               dict(nsl=one(0)), dict(nsl=one((1 << 31) + 1))):
        assert call(**kw) == _capi.VK_EINVAL, kw
    for args in ((None, 1, 64, C.byref(b)), (nsl, 0, 64, C.byref(b)), (nsl, 1, 63, C.byref(b)), (nsl, 1, (1 << 20) + 1, C.byref(b)),
                 (nsl, 1, 64, None), (one(0), 1, 64, C.byref(b))):
        assert L.vk_sketch_workspace_size(*args) == _capi.VK_EINVAL, args
    with pytest.raises(ValueError):
        eng.sketch_tables(keys, counts, [0], [1024], status, 63, 1)
    with pytest.raises(ValueError):
        eng.sketch_tables(keys, counts, [0], [1024], status, 64, 0)
    with pytest.raises(ValueError):
        eng.sketch_tables(keys, counts, [1], [1024], status, 64, 1)


# ---------------------------------------------------------------------- pairs --

def test_pairs_of_the_seam_cases(eng):
    """every sketch of tests/sketch_cases.seam_pairs against every other: 28 x 28 pairs, the named ones among them"""
    s = 64
    cases = KC.seam_pairs(s)
    sketches = [x for _, a, b in cases for x in (a, b)]
    rows, lens = KC.pair_rows(sketches, s)
    assert {0, 1, s - 1, s} <= set(lens.tolist()) and any((len(a) + len(b)) % 64 for _, a, b in cases)
    shared, seen = eng.sketch_pairs(rows, lens, rows, lens, s)   # (q is r)
    assert shared.dtype == np.uint32 and shared.shape == (len(sketches), len(sketches))
    for i, a in enumerate(sketches):
        for j, b in enumerate(sketches):
            assert (int(shared[i, j]), int(seen[i, j])) == R.pair_loop(a, b, s), (i, j)
    for n, (name, a, b) in enumerate(cases):
        assert (int(shared[2 * n, 2 * n + 1]), int(seen[2 * n, 2 * n + 1])) == R.pair_np(a, b, s), name
    assert (shared[0, 0], seen[0, 0]) == (0, 0)   # empty against empty


def test_pairs_9_by_31_of_larger_sketches(eng):
    """s = 1,000, sketches drawn from a pool so that they overlap, lengths from 0 to s: segments of up to 32 values"""
    rng = random.Random(8)
    s = 1000
    pool = KC.spread(rng, 3000)
    def draw(n):
        return sorted(rng.sample(pool, n))
    q = [draw(n) for n in (0, 1, 31, 500, 999, 1000, 1000, 777, 64)]
    r = [draw(rng.choice((0, 1, 999, 1000, rng.randrange(2, 999)))) for _ in range(29)] + [q[5], q[4]]
    qr, ql = KC.pair_rows(q, s)
    rr, rl = KC.pair_rows(r, s)
    shared, seen = eng.sketch_pairs(qr, ql, rr, rl, s)
    assert shared.shape == (9, 31)
    for i, a in enumerate(q):
        for j, b in enumerate(r):
            assert (int(shared[i, j]), int(seen[i, j])) == R.pair_np(a, b, s), (i, j)
    assert (shared[5, 29], seen[5, 29]) == (1000, 1000)


def test_pairs_error_codes(eng):
    import torch
    L, p = eng.L, eng._ptr
    rows = torch.full((2, 64), -1, dtype=torch.int64, device=eng.device)
    lens = torch.zeros(2, dtype=torch.int64, device=eng.device)
    out = torch.zeros((2, 2), dtype=torch.int32, device=eng.device)

    def call(ctx=eng.ctx, q=p(rows), ql=p(lens), nq=2, r=p(rows), rl=p(lens), nr=2, s=64, sh=p(out), se=p(out)):
        return L.vk_sketch_pairs_device(ctx, q, ql, nq, r, rl, nr, s, sh, se)
    assert call() == _capi.VK_OK
    assert eng.L.vk_ctx_sync(eng.ctx) == _capi.VK_OK
    for kw in (dict(ctx=None), dict(q=None), dict(ql=None), dict(r=None), dict(rl=None), dict(sh=None), dict(se=None), dict(nq=0),
               dict(nr=0), dict(s=63), dict(s=(1 << 20) + 1), dict(nq=(1 << 20) + 1), dict(nr=(1 << 20) + 1),
               dict(nq=1 << 20, nr=(1 << 12) + 1)):
        assert call(**kw) == _capi.VK_EINVAL, kw
    with pytest.raises(ValueError):
        eng.sketch_pairs(np.zeros((2, 63), dtype=np.uint64), [0, 0], np.zeros((2, 63), dtype=np.uint64), [0, 0], 64)
    with pytest.raises(ValueError):
        eng.sketch_pairs(np.zeros((2, 64), dtype=np.uint64), [0, 65], np.zeros((2, 64), dtype=np.uint64), [0, 0], 64)
