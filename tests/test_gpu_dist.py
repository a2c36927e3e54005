"""`compare`'s device call on the GPU (ImageEngine.neighbours, vk_dist_device) against the rule in NumPy
(tests/dist_ref.py): idx, d2 and the matrix equal, exactly, on every case of tests/dist_cases.py (its docstring names the
paths: grids of several tiles both ways, slices, a wavefront's second look with more than one entry per lane); strip
seams (VKIMG_DIST_STRIP), also across grids with several reference tiles and rows of several entries per thread; the
second look run twice on copies; self mode; refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import dist_cases as DC
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in DC.all_cases()]


@pytest.fixture(scope="module")
def dist_engines():
    """"small" | "default" -> an ImageEngine whose context was made with VKIMG_DIST_STRIP = 64 or without it."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(strip):
        if strip not in cache:
            old = os.environ.pop("VKIMG_DIST_STRIP", None)
            try:
                if strip == "small":
                    os.environ["VKIMG_DIST_STRIP"] = "64"
                cache[strip] = ImageEngine(k=7, mapping="cgr", device=0)
            finally:
                os.environ.pop("VKIMG_DIST_STRIP", None)
                if old is not None:
                    os.environ["VKIMG_DIST_STRIP"] = old
        return cache[strip]
    yield get
    for e in cache.values():
        e.close()


def on_device(eng, a):
    import torch
    return torch.from_numpy(np.array(a)).to(eng.device)


def run(eng, c):
    q = on_device(eng, c.q)
    r = q if c.r is c.q else on_device(eng, c.r)
    idx, d2, m = eng.neighbours(q, r, n=c.n, qgroup=c.qgroup, rgroup=c.rgroup, matrix=True)
    return idx, d2, m.cpu().numpy().view(np.uint64)


def check(got, name, what=""):
    em, eidx, ed2 = DC.expected(name)
    idx, d2, m = got
    assert idx.dtype == np.uint32 and d2.dtype == np.uint64 and idx.shape == eidx.shape and m.shape == em.shape
    assert np.array_equal(m, em), (name, what, "matrix", np.argwhere(m != em)[:4])
    assert np.array_equal(idx, eidx), (name, what, "idx", np.argwhere(idx != eidx)[:4])
    assert np.array_equal(d2, ed2), (name, what, "d2", np.argwhere(d2 != ed2)[:4])


@pytest.mark.parametrize("name", NAMES)
def test_every_case(dist_engines, name):
    check(run(dist_engines("default"), DC.by_name(name)), name)


def test_black_against_white_at_512_squared(dist_engines):
    idx, d2, m = run(dist_engines("default"), DC.by_name("extremes_262144"))
    assert int(m[0, 1]) == DC.D2_BLACK_WHITE_512 and int(m[0, 0]) == 0 and int(m[1, 1]) == 0


@pytest.mark.parametrize("name", ["tile_edges_257x63", "tile_edges_129x31", "structured", "ties", "groups_mixed", "grid_257x385",
                                  "grid_structured_300x200", "select_1000"])
def test_strips_of_64_rows_give_the_same(dist_engines, name):
    """Four seams across the 257 queries of tile_edges; strips that are no multiple of the tile; in the grids every strip
    is a launch of its own over 4 or 2 reference tiles."""
    assert name in NAMES
    small = run(dist_engines("small"), DC.by_name(name))
    check(small, name, "VKIMG_DIST_STRIP=64")
    for a, b in zip(small, run(dist_engines("default"), DC.by_name(name))):
        assert np.array_equal(a, b)


def test_the_second_look_keeps_no_state_between_calls(dist_engines):
    """select_ties_16700 twice, on copies: nothing of the look through a winner's entries depends on an earlier call."""
    import torch
    eng, c = dist_engines("default"), DC.by_name("select_ties_16700")
    q, r = on_device(eng, c.q), on_device(eng, c.r)
    outs = []
    for _ in range(2):
        idx, d2, m = eng.neighbours(q.clone(), r.clone(), n=c.n, matrix=True)
        outs.append((idx, d2, m.cpu().numpy().view(np.uint64)))
    assert torch.equal(q.cpu(), torch.from_numpy(np.array(c.q))) and torch.equal(r.cpu(), torch.from_numpy(np.array(c.r)))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    check(outs[1], c.name, "second call")


def test_without_the_matrix(dist_engines):
    eng, c = dist_engines("default"), DC.by_name("pad")
    idx, d2 = eng.neighbours(on_device(eng, c.q), on_device(eng, c.r), n=c.n)
    _, eidx, ed2 = DC.expected("pad")
    assert np.array_equal(idx, eidx) and np.array_equal(d2, ed2)


def test_images_as_squares(dist_engines):
    eng, c = dist_engines("default"), DC.by_name("pad")
    idx, d2 = eng.neighbours(on_device(eng, c.q.reshape(5, 23, 23)), on_device(eng, c.r.reshape(7, 23, 23)), n=c.n)
    _, eidx, ed2 = DC.expected("pad")
    assert np.array_equal(idx, eidx) and np.array_equal(d2, ed2)


def test_self_mode_is_symmetric_with_a_zero_diagonal(dist_engines):
    import dist_ref
    eng = dist_engines("default")
    x = DC.by_name("tile_edges_129x31").q
    q = on_device(eng, x)
    idx, d2, m = eng.neighbours(q, q, n=3, matrix=True)
    m = m.cpu().numpy().view(np.uint64)
    assert np.array_equal(m, m.T) and not m.diagonal().any()
    em = dist_ref.matrix(x, x)
    assert np.array_equal(m, em)
    eidx, ed2 = dist_ref.neighbours(em, 3)
    assert np.array_equal(idx, eidx) and np.array_equal(d2, ed2)
    assert idx[:, 0].tolist() == list(range(len(x)))   # (without groups an image is its own nearest)


@pytest.mark.parametrize("n", [0, 65])
def test_a_neighbour_count_outside_1_to_64_is_refused(dist_engines, n):
    eng, c = dist_engines("default"), DC.by_name("pad")
    with pytest.raises(_capi.VkError) as e:
        eng.neighbours(on_device(eng, c.q), on_device(eng, c.r), n=n)
    assert e.value.status == _capi.VK_EINVAL


def test_wrong_arguments_return_error_codes_and_write_nothing(dist_engines):
    import torch
    eng, c = dist_engines("default"), DC.by_name("pad")
    q, r = on_device(eng, c.q), on_device(eng, c.r)
    nq, nr, p, n = 5, 7, 529, 4
    need = C.c_uint64()
    size = eng.L.vk_dist_workspace_size
    assert size(nq, nr, p, n, 0, C.byref(need)) == _capi.VK_OK and need.value > 0
    for bad in ((nq, nr, 0, n), (nq, nr, p, 0), (nq, nr, p, 65), (0, nr, p, n), (nq, 0, p, n), (nq, (1 << 30) + 1, p, n),
                (nq, nr, (1 << 20) + 1, n)):
        assert size(*bad, 0, C.byref(need)) == _capi.VK_EINVAL, bad
    assert size(nq, nr, p, n, 0, C.byref(need)) == _capi.VK_OK
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=eng.device)
    idx = torch.full((nq, 64), 7, dtype=torch.int32, device=eng.device)
    d2 = torch.full((nq, 64), 7, dtype=torch.int64, device=eng.device)

    def call(nq=nq, nr=nr, p=p, n=n, ws_bytes=int(need.value), q=q, idx=idx):
        return eng.L.vk_dist_device(eng.ctx, eng._ptr(q) if q is not None else None, nq, eng._ptr(r), nr, p, None, None, n,
                                    eng._ptr(idx) if idx is not None else None, eng._ptr(d2), None, eng._ptr(ws), ws_bytes)

    for kw in (dict(n=0), dict(n=65), dict(p=0), dict(nq=0), dict(nr=0), dict(ws_bytes=int(need.value) - 1), dict(q=None), dict(idx=None)):
        assert call(**kw) == _capi.VK_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((idx == 7).all()) and bool((d2 == 7).all())   # (nothing was written)
    assert call() == _capi.VK_OK
    torch.cuda.synchronize()
    _, eidx, ed2 = DC.expected("pad")
    got = idx.cpu().numpy().view(np.uint32).reshape(-1)[:nq * n].reshape(nq, n)   # (rows of n slots, packed)
    assert np.array_equal(got, eidx[:, :n])
