"""The per-block pair counts on the GPU (vk_sketch_pair_blocks_device, ImageEngine.sketch_pair_blocks) against the loop of
tests/tree_ref.py: every sketch of tests/sketch_cases.seam_pairs against every other with `q is r` (lengths 0, 1, s - 1
and s; identical, disjoint and interleaved sketches; a common value at every segment seam), 9 x 31 larger sketches whose
union passes s (the stop falls inside a lane's segment), the 64 counts summing to vk_sketch_pairs_device's outputs, and the
error codes."""
import functools
import random

import numpy as np
import pytest

import sketch_cases as KC
import tree_ref as R
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from varkoder_amd.engine import ImageEngine
    e = ImageEngine(k=7, mapping="cgr", device=0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def seam_sketches(s=64):
    return [x for _, a, b in KC.seam_pairs(s) for x in (a, b)]


def test_blocks_of_the_seam_cases(eng):
    s = 64
    sketches = seam_sketches(s)
    rows, lens = KC.pair_rows(sketches, s)
    assert {0, 1, s - 1, s} <= set(lens.tolist())
    shared, seen = eng.sketch_pair_blocks(rows, lens, rows, lens, s)   # (q is r)
    assert shared.dtype == np.uint32 and shared.shape == seen.shape == (len(sketches), len(sketches), 64)
    for i, a in enumerate(sketches):
        for j, b in enumerate(sketches):
            want = R.pair_blocks_loop(a, b, s)
            assert shared[i, j].tolist() == want[0] and seen[i, j].tolist() == want[1], (i, j)
    assert not shared[0, 0].any() and not seen[0, 0].any()   # empty against empty
    plain = eng.sketch_pairs(rows, lens, rows, lens, s)
    assert np.array_equal(shared.sum(axis=-1), plain[0]) and np.array_equal(seen.sum(axis=-1), plain[1])


def test_blocks_9_by_31_of_larger_sketches(eng):
    """s = 1,000, overlapping sketches of lengths 0 to s, q and r different sets"""
    rng = random.Random(8)
    s = 1000
    pool = KC.spread(rng, 3000)

    def draw(n):
        return sorted(rng.sample(pool, n))
    q = [draw(n) for n in (0, 1, 31, 500, 999, 1000, 1000, 777, 64)]
    r = [draw(rng.choice((0, 1, 999, 1000, rng.randrange(2, 999)))) for _ in range(29)] + [q[5], q[4]]
    qr, ql = KC.pair_rows(q, s)
    rr, rl = KC.pair_rows(r, s)
    shared, seen = eng.sketch_pair_blocks(qr, ql, rr, rl, s)
    assert shared.shape == (9, 31, 64)
    for i, a in enumerate(q):
        for j, b in enumerate(r):
            want = R.pair_blocks_loop(a, b, s)
            assert shared[i, j].tolist() == want[0] and seen[i, j].tolist() == want[1], (i, j)
    assert int(shared[5, 29].sum()) == 1000 == int(seen[5, 29].sum())
    plain = eng.sketch_pairs(qr, ql, rr, rl, s)
    assert np.array_equal(shared.sum(axis=-1), plain[0]) and np.array_equal(seen.sum(axis=-1), plain[1])


def test_blocks_error_codes(eng):
    import torch
    L, p = eng.L, eng._ptr
    rows = torch.full((2, 64), -1, dtype=torch.int64, device=eng.device)
    lens = torch.zeros(2, dtype=torch.int64, device=eng.device)
    out = torch.zeros((2, 2, 64), dtype=torch.int32, device=eng.device)

    def call(ctx=eng.ctx, q=p(rows), ql=p(lens), nq=2, r=p(rows), rl=p(lens), nr=2, s=64, sh=p(out), se=p(out)):
        return L.vk_sketch_pair_blocks_device(ctx, q, ql, nq, r, rl, nr, s, sh, se)
    assert call() == _capi.VK_OK
    assert L.vk_ctx_sync(eng.ctx) == _capi.VK_OK
    for kw in (dict(ctx=None), dict(q=None), dict(ql=None), dict(r=None), dict(rl=None), dict(sh=None), dict(se=None), dict(nq=0),
               dict(nr=0), dict(s=63), dict(s=(1 << 20) + 1), dict(nq=(1 << 20) + 1), dict(nr=(1 << 20) + 1),
               dict(nq=1 << 13, nr=(1 << 13) + 1)):
        assert call(**kw) == _capi.VK_EINVAL, kw
    with pytest.raises(ValueError):
        eng.sketch_pair_blocks(np.zeros((2, 63), dtype=np.uint64), [0, 0], np.zeros((2, 63), dtype=np.uint64), [0, 0], 64)
    with pytest.raises(ValueError):
        eng.sketch_pair_blocks(np.zeros((2, 64), dtype=np.uint64), [0, 65], np.zeros((2, 64), dtype=np.uint64), [0, 0], 64)
