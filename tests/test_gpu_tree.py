"""Neighbour joining on the GPU (vk_tree_nj_device, ImageEngine.nj) against tests/tree_ref.py, bit for bit: n = 3 (no
join), 4, 5, 64 and 65; n = 257 (a row crosses a partial stride, several strips, odd rows whose 16-byte pairs begin a
column early); n = 600 (two column tiles, 38 strips, the fold of their partials); the tie matrices; calls of 5
different matrices of which one is invalid -- a NaN, a negative entry, an asymmetric pair, a non-zero diagonal -- whose
status is set and record zeroed while the others are exact; the same matrix 3 times; two calls on copies; every VK_EINVAL.

The second column tile and the odd rows: n = 511, 512 and 513 at an even base (513 is the first size whose odd rows reach
tile 1: its lane 0 holds columns 511 and 512, takes R[511] from the slot in front of the tile's own, and column 1023 would
be the next tile's); two trees of n = 513 and 601 in one call (the second at an odd multiple of 8 bytes, the parity of its
rows alternating the other way); an even n at an odd base (every row odd: at n = 512 column 511 is met in the extra tile
alone; also 64, 65 and 600, one tree and two).  Ties across workgroups: all ones at 513 and 600 leaves (every step a tie
of every pair, through the workgroups' minima, the partials and the join's strided fold), and
tree_cases.exact_cherries of 600 leaves with equal cherries in different tiles and strips, the winner once in tile 1 and
once in tile 0.  In each of these runs later joins retire all 16 rows of a strip (a search workgroup with no row
listed) and leave blocks wholly below the diagonal (skipped): both paths are entered without a test of their own."""
import ctypes as C
import functools

import numpy as np
import pytest

import tree_cases as TC
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
def want(kind, n, seed):
    """(D, the rule's (status, nodes, lengths)): computed once and shared."""
    D = {"additive": lambda: TC.additive(n, seed)[0], "noisy": lambda: TC.noisy(n, seed), "arbitrary": lambda: TC.arbitrary(n, seed),
         "ones": lambda: TC.ones(n), "three_identical": lambda: TC.three_identical(n, seed),
         "cherries": lambda: TC.exact_cherries(n, CHERRIES[seed], seed)}[kind]()
    D.setflags(write=False)
    return D, R.nj_np(D)


# exact_cherries' pairs by seed: columns 40 | 520, 590 lie in tiles 0 | 1; rows 3, 4 | 17 | 530 in strips 0 | 1 | 33
CHERRIES = {1: ((3, 520), (17, 40), (530, 590)),    # the winner in tile 1, a tile-0 pair of a later strip beaten
            2: ((3, 40), (17, 520), (530, 590)),    # the mirror: the winner in tile 0
            3: ((3, 520), (4, 40), (530, 590))}     # winner and runner-up in one strip, tiles 1 and 0


def same(got, i, ref):
    status, nodes, lengths = got
    assert int(status[i]) == ref[0]
    assert np.array_equal(nodes[i], ref[1])
    assert lengths[i].tobytes() == np.asarray(ref[2]).tobytes()   # bit for bit


@pytest.mark.parametrize("n", [3, 4, 5, 64, 65])
def test_small_trees(eng, n):
    for kind, seed in (("additive", n), ("noisy", 10 + n), ("arbitrary", 20 + n)):
        D, ref = want(kind, n, seed)
        got = eng.nj(D)
        assert got[1].shape == (1, R.record_len(n)) and got[1].dtype == np.uint32 and got[2].dtype == np.float64
        same(got, 0, ref)
    assert ref[0] == 0


def test_257_leaves_cross_a_partial_stride_and_fill_several_strips(eng):
    for kind in ("noisy", "arbitrary"):
        D, ref = want(kind, 257, 3)
        same(eng.nj(D), 0, ref)
    # two trees of an odd n: the second lies at an odd multiple of 8 bytes, and every row's parity flips
    D2, ref2 = want("noisy", 257, 4)
    got = eng.nj(np.stack([D, D2]))
    same(got, 0, ref)
    same(got, 1, ref2)


def test_600_leaves_several_workgroups_per_tree_and_the_partial_fold(eng):
    D, ref = want("noisy", 600, 5)
    same(eng.nj(D), 0, ref)


def test_ties_go_to_the_smaller_i_then_the_smaller_j(eng):
    D, ref = want("ones", 5, 0)
    assert ref[1][:4].tolist() == [0, 1, 0, 2]
    same(eng.nj(D), 0, ref)
    D, ref = want("ones", 70, 0)
    same(eng.nj(D), 0, ref)
    D, ref = want("three_identical", 7, 5)
    same(eng.nj(D), 0, ref)


def at_odd_base(eng, mats):
    """The matrices on the device in one block that begins at an odd multiple of 8 bytes."""
    import torch
    t, n = len(mats), len(mats[0])
    flat = torch.zeros(1 + t * n * n + 1, dtype=torch.float64, device=eng.device)
    dd = flat[1:1 + t * n * n].view(t, n, n)
    dd.copy_(torch.from_numpy(np.stack(mats)))
    assert dd.data_ptr() % 16 == 8 and dd.is_contiguous()
    return dd


@pytest.mark.parametrize("n", [511, 512, 513])
def test_rows_around_the_second_column_tile(eng, n):
    D, ref = want("noisy", n, 5)
    same(eng.nj(D), 0, ref)


@pytest.mark.parametrize("n", [513, 601])
@pytest.mark.parametrize("kind", ["noisy", "arbitrary"])
def test_two_trees_of_an_odd_n_past_one_tile(eng, kind, n):
    """The second tree lies at an odd base: the rows whose pairs begin a column early are the even ones there."""
    (D, ref), (D2, ref2) = want(kind, n, 5), want(kind, n, 4)
    got = eng.nj(np.stack([D, D2]))
    same(got, 0, ref)
    same(got, 1, ref2)


@pytest.mark.parametrize("n", [64, 65, 512, 600])
def test_a_matrix_at_an_odd_multiple_of_8_bytes(eng, n):
    """An even n there makes every row odd; one tree, then two."""
    (D, ref), (D2, ref2) = want("noisy", n, 5), want("noisy", n, 4)
    same(eng.nj_device(at_odd_base(eng, [D])), 0, ref)
    got = eng.nj_device(at_odd_base(eng, [D, D2]))
    same(got, 0, ref)
    same(got, 1, ref2)


@pytest.mark.parametrize("n", [513, 600])
def test_all_ones_tie_across_every_workgroup(eng, n):
    D, ref = want("ones", n, 0)
    assert ref[1][:4].tolist() == [0, 1, 0, 2]
    same(eng.nj(D), 0, ref)


@pytest.mark.parametrize("seed", sorted(CHERRIES))
def test_equal_cherries_in_different_tiles_and_strips(eng, seed):
    D, ref = want("cherries", 600, seed)
    pairs = sorted(CHERRIES[seed])
    assert ref[0] == 0 and ref[1][:6].reshape(3, 2).tolist() == [list(p) for p in pairs]   # the smaller i, then the smaller j
    assert ref[2][:6].tolist() == [2.0, 4.0] * 3 and np.array_equal(ref[2], np.round(ref[2]))   # integers: the ties are real
    same(eng.nj(D), 0, ref)
    if seed == 1:   # every row odd as well
        same(eng.nj_device(at_odd_base(eng, [D])), 0, ref)


@pytest.mark.parametrize("kind", ["nan", "negative", "asymmetric", "diagonal", "inf", "too_large"])
def test_an_invalid_matrix_disturbs_no_other(eng, kind):
    n = 9
    good = [want(k, n, s) for k, s in (("additive", 1), ("noisy", 2), ("arbitrary", 3), ("ones", 0))]
    bad = TC.invalid(kind, n)
    assert R.nj_np(bad)[0] == R.BAD_VALUE and R.nj_loop(bad)[0] == R.BAD_VALUE
    mats = [good[0][0], good[1][0], bad, good[2][0], good[3][0]]
    status, nodes, lengths = eng.nj(np.stack(mats))
    assert status.tolist() == [0, 0, _capi.VK_TREE_BAD_VALUE, 0, 0]
    assert not nodes[2].any() and lengths[2].tobytes() == bytes(8 * R.record_len(n))
    for at, g in zip((0, 1, 3, 4), good):
        same((status, nodes, lengths), at, g[1])


def test_the_same_matrix_three_times_and_two_calls_on_copies(eng):
    D, ref = want("noisy", 65, 75)
    got = eng.nj(np.stack([D, D, D]))
    for i in range(3):
        same(got, i, ref)
    again = eng.nj(np.stack([D.copy(), D.copy(), D.copy()]))
    assert np.array_equal(got[1], again[1]) and got[2].tobytes() == again[2].tobytes()


def test_the_device_matrix_is_the_callers_to_lose(eng):
    import torch
    D, ref = want("noisy", 64, 74)
    dd = torch.from_numpy(D.copy()[None]).to(eng.device)
    same(eng.nj_device(dd), 0, ref)


def test_error_codes(eng):
    import torch
    n, t = 8, 2
    L = eng.L
    size = C.c_uint64()
    assert L.vk_tree_workspace_size(n, t, C.byref(size)) == _capi.VK_OK and size.value > 0
    assert L.vk_tree_workspace_size(n, t, None) == _capi.VK_EINVAL
    for bn, bt in ((2, 1), (_capi.VK_TREE_MAX_LEAVES + 1, 1), (n, 0), (n, _capi.VK_TREE_MAX_TREES + 1)):
        assert L.vk_tree_workspace_size(bn, bt, C.byref(size)) == _capi.VK_EINVAL
    assert L.vk_tree_workspace_size(n, t, C.byref(size)) == _capi.VK_OK
    rec = R.record_len(n)
    d = torch.zeros((t, n, n), dtype=torch.float64, device=eng.device)
    nodes = torch.zeros((t, rec), dtype=torch.int32, device=eng.device)
    lengths = torch.zeros((t, rec), dtype=torch.float64, device=eng.device)
    status = torch.zeros((t,), dtype=torch.int32, device=eng.device)
    ws = torch.zeros(max(size.value, 256), dtype=torch.uint8, device=eng.device)
    p = eng._ptr
    ok = [eng.ctx, p(d), n, t, p(nodes), p(lengths), p(status), p(ws), size.value]
    assert L.vk_tree_nj_device(*ok) == _capi.VK_OK
    assert L.vk_ctx_sync(eng.ctx) == _capi.VK_OK
    for at in (0, 1, 4, 5, 6, 7):
        args = list(ok)
        args[at] = None
        assert L.vk_tree_nj_device(*args) == _capi.VK_EINVAL, at
    for at, v in ((2, 2), (2, _capi.VK_TREE_MAX_LEAVES + 1), (3, 0), (3, _capi.VK_TREE_MAX_TREES + 1), (8, size.value - 1)):
        args = list(ok)
        args[at] = v
        assert L.vk_tree_nj_device(*args) == _capi.VK_EINVAL, (at, v)
    with pytest.raises(ValueError):
        eng.nj(np.zeros((2, 2)))
    with pytest.raises(ValueError):
        eng.nj(np.zeros((3, 4)))
