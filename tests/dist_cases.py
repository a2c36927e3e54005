"""Named cases of `compare`'s device call (the rule: tests/dist_ref.py): small inputs at which the tile kernel, the
slice and the selection can go wrong.  Shared by the host emulation (tests/test_dist_emulation.py) and the GPU tests
(tests/test_gpu_dist.py).  Every case is a few seconds of NumPy at most.

The paths they enter: tile_edges_* a partial tile of queries or of references (each edge size once as nq, once as nr);
grid_* more than one tile of queries AND of references at once, the two counts different (3 x 4, 3 x 2), so that the
decode of the one-dimensional grid into a tile's corner matters -- grid_structured_300x200 is asymmetric in i and j, and
`expected` asserts that exchanging the roles of the two indices changes every pair of tiles; k_steps_* the K steps;
extremes_* the fold of a slice at the largest values; slice_* random images that end one pixel, one K step and two
slices past the first slice; ties, groups_*, n_values_* the selection with one entry per thread; select_1000 three or
four entries per thread; select_ties_16700 and select_one_thread_17000 more than 64 x 256 references, so that a lane
of the wavefront that looks through the winner's entries again has a second entry -- in the first the order within
long runs of equal distances rests on j alone and a query's copies lie 16,384 apart in one thread, in the second all 64
neighbours of a query belong to thread 5 and three of them lie past the stride (`expected` asserts each layout);
select_groups_1000 a group that leaves 40 references, one that excludes none, and no group, over several entries per
thread."""
import collections
import functools

import numpy as np

NO_GROUP = NO_IDX = 0xFFFFFFFF
Case = collections.namedtuple("Case", "name q r n qgroup rgroup")   # q, r: uint8 [n, P]; groups: uint32 arrays or None

EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
K_STEPS = (1, 63, 64, 65, 127, 129, 4095, 4097)
EXTREME_PIXELS = (262144, 131769)   # 512^2 and 363^2
SLICE = 65536                       # kDistSlice
SLICE_PIXELS = (SLICE + 1, SLICE + 128, 2 * SLICE + 1)   # a pixel and a whole K step into the second slice; three slices
SEL_THREADS, SEL_STRIDE = 256, 64 * 256                  # kDistSelThreads; the stride of a lane that looks again
D2_BLACK_WHITE_512 = 17045913600    # 255^2 * 512^2


def _rng(name):
    return np.random.default_rng(sum(name.encode()) * 7919 + len(name))


def _random(name, nq, nr, p, n=10):
    g = _rng(name)
    return Case(name, g.integers(0, 256, (nq, p), dtype=np.uint8), g.integers(0, 256, (nr, p), dtype=np.uint8), n, None, None)


def _pad():
    return [_random("pad", 5, 7, 529)]


def _tile_edges():
    # pairs, not the cross product: every value once as nq and once as nr (nr = the value five places on)
    return [_random("tile_edges_%dx%d" % (nq, EDGES[(i + 5) % len(EDGES)]), nq, EDGES[(i + 5) % len(EDGES)], 1024)
            for i, nq in enumerate(EDGES)]


def _k_steps():
    return [_random("k_steps_%d" % p, 33, 33, p) for p in K_STEPS]


def _structured():
    i, j, p = np.arange(70)[:, None], np.arange(45)[:, None], np.arange(8281)[None, :]
    return [Case("structured", ((37 * i + 11 * p) % 256).astype(np.uint8), ((91 * j + 5 * p + 3) % 256).astype(np.uint8), 10, None, None)]


def _grids():
    i, j, p = np.arange(300)[:, None], np.arange(200)[:, None], np.arange(256)[None, :]
    return [_random("grid_257x385", 257, 385, 128),
            Case("grid_structured_300x200", ((37 * i + 11 * p) % 256).astype(np.uint8), ((91 * j + 5 * p + 3) % 256).astype(np.uint8), 10,
                 None, None)]


def _slices():
    return [_random("slice_%d" % p, 5, 7, p, 4) for p in SLICE_PIXELS]


def _extremes():
    out = []
    for p in EXTREME_PIXELS:
        checker = ((np.arange(p) % 2) * 255).astype(np.uint8)
        q = np.stack([np.zeros(p, np.uint8), np.full(p, 255, np.uint8), np.full(p, 128, np.uint8), checker])
        r = np.stack([np.zeros(p, np.uint8), np.full(p, 255, np.uint8), np.full(p, 128, np.uint8), 255 - checker])
        out.append(Case("extremes_%d" % p, q, r, 4, None, None))
    return out


def _ties():
    g = _rng("ties")
    r = g.integers(0, 256, (45, 77), dtype=np.uint8)
    r[17] = r[3]
    r[40] = r[3]
    q = g.integers(0, 256, (6, 77), dtype=np.uint8)
    q[0] = r[3]                # three references at distance 0
    q[1] = r[3]
    q[1, 5] ^= 1               # and at distance 1
    q[2] = r[9]                # a reference equal to a query
    few = Case("ties_fill", q.copy(), r[[3, 17, 40]].copy(), 10, None, None)   # nr = 3 < N
    return [Case("ties", q, r, 5, None, None), few]


def _groups():
    g = _rng("groups")
    q, r = g.integers(0, 256, (6, 64), dtype=np.uint8), g.integers(0, 256, (9, 64), dtype=np.uint8)
    u = lambda v: np.array(v, dtype=np.uint32)   # noqa: E731
    return [Case("groups_mixed", q, r, 5, u([0, 1, 2, 3, NO_GROUP, 7]), u([0, 0, 1, 1, 2, 2, 2, 3, 3])),
            Case("groups_whole_set", q, r, 4, u([5, NO_GROUP, 5, 1, NO_GROUP, 5]), u([5] * 9)),
            Case("groups_self", r, r, 10, u([0, 0, 1, 1, 2, 2, 2, 3, 3]), u([0, 0, 1, 1, 2, 2, 2, 3, 3]))]


def _n_values():
    return [_random("n_values_%d" % n, 9, 100, 100, n) for n in (1, 10, 64)]


def _select():
    u = lambda v: np.array(v, dtype=np.uint32)   # noqa: E731
    out = [_random("select_1000", 3, 1000, 16, 64)]
    # pixels 0 .. 3: d2 <= 144, so thousands of the references share each distance.  Copies of queries 0 and 1 one stride
    # apart: both belong to one thread, the second is the second entry of the lane that looks again
    g = _rng("select_ties_16700")
    q, r = g.integers(0, 4, (3, 16), dtype=np.uint8), g.integers(0, 4, (16700, 16), dtype=np.uint8)
    r[7] = r[7 + SEL_STRIDE] = q[0]
    r[300] = r[300 + SEL_STRIDE] = q[1]
    out.append(Case("select_ties_16700", q, r, 64, None, None))
    # query 0's 64 nearest all in thread 5: its copy with d pixels changed by one (d2 = d) is entry (37 d + 30) % 67 of the
    # thread's 67, so entries 64, 65 and 66 (past one stride) hold d = 48, 10 and 39 -- none is the thread's first answer,
    # each is found only when a lane looks again and reads its second entry -- and j does not rise with d
    g = _rng("select_one_thread_17000")
    q, r = g.integers(0, 256, (3, 64), dtype=np.uint8), g.integers(0, 256, (17000, 64), dtype=np.uint8)
    for d in range(64):
        r[5 + SEL_THREADS * ((37 * d + 30) % 67)] = q[0]
        r[5 + SEL_THREADS * ((37 * d + 30) % 67), :d] ^= 1
    out.append(Case("select_one_thread_17000", q, r, 64, None, None))
    g = _rng("select_groups_1000")
    q, r = g.integers(0, 256, (3, 16), dtype=np.uint8), g.integers(0, 256, (1000, 16), dtype=np.uint8)
    rgroup = np.full(1000, 1, dtype=np.uint32)
    rgroup[g.choice(1000, 40, replace=False)] = 2
    out.append(Case("select_groups_1000", q, r, 64, u([1, 9, NO_GROUP]), rgroup))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, built once; the arrays are read-only."""
    cases = (_pad() + _tile_edges() + _k_steps() + _structured() + _extremes() + _ties() + _groups() + _n_values() + _grids() +
             _slices() + _select())
    for c in cases:
        for a in (c.q, c.r, c.qgroup, c.rgroup):
            if a is not None:
                a.setflags(write=False)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(matrix, idx, d2) of a case by tests/dist_ref.py: computed once, left unchanged."""
    import dist_ref
    c = by_name(name)
    m = dist_ref.matrix(c.q, c.r)
    idx, d2 = dist_ref.neighbours(m, c.n, c.qgroup, c.rgroup)
    for a in (m, idx, d2):
        a.setflags(write=False)
    _check_layout(c, m, idx, d2)
    return m, idx, d2


def _nearest(row, n):
    """The n nearest of one row of the matrix, without groups."""
    return np.argsort(row, kind="stable")[:n].astype(np.uint32)


def _longest_run(row):
    cuts = np.flatnonzero(np.diff(row.astype(np.int64)) != 0)
    return int(np.diff(np.concatenate([[-1], cuts, [len(row) - 1]])).max())


def _check_layout(c, m, idx, d2):
    """What a case was built to hold, asserted of the rule's own answer."""
    if c.name == "grid_structured_300x200":
        # a decode that exchanges i0 and j0 computes d2(q[j], r[i]): where both exist that is the transpose, and it must
        # differ in every pair of tiles (so also in the tiles on the diagonal)
        sq = m[:200, :200]
        for a in range(0, 200, 128):
            for b in range(0, 200, 128):
                assert (sq[a:a + 128, b:b + 128] != sq.T[a:a + 128, b:b + 128]).any(), (c.name, a, b)
        assert (sq != sq.T).mean() > 0.9, c.name
        # (37 x 128 and 91 x 128 are both 128 mod 256 and P is a whole period: tile (1, 1) repeats tile (0, 0).  A tile
        # written to another's place is told by the random grid_257x385, this case tells i from j)
    if c.name == "select_1000":
        assert len(c.r) // SEL_THREADS == 3 and len(c.r) % SEL_THREADS   # (3 or 4 entries a thread)
    if c.name == "select_ties_16700":
        assert len(c.r) > SEL_STRIDE and c.r.max() <= 3
        assert max(_longest_run(row) for row in d2) >= 10, c.name          # the order rests on j alone
        for i, j in ((0, 7), (1, 300)):                                    # a thread's first entry, then its lane's second
            assert idx[i, :2].tolist() == [j, j + SEL_STRIDE] and not d2[i, :2].any(), (c.name, i)
    if c.name == "select_one_thread_17000":
        assert (idx[0] % SEL_THREADS == 5).all() and d2[0].tolist() == list(range(64)), c.name
        assert [idx[0, d] for d in (48, 10, 39)] == [5 + SEL_THREADS * k for k in (64, 65, 66)], c.name   # past one stride
        assert (np.diff(idx[0].astype(np.int64)) < 0).any(), c.name
    if c.name == "select_groups_1000":
        assert (idx[0, 40:] == NO_IDX).all() and (c.rgroup[idx[0, :40]] == 2).all(), c.name   # the fill starts at rank 40
        assert not (c.rgroup == c.qgroup[1]).any() and c.qgroup[2] == NO_GROUP
        for i in (1, 2):
            assert np.array_equal(idx[i], _nearest(m[i], c.n)), (c.name, i)
