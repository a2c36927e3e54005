"""Named cases of `compare`'s device call (the rule: tests/dist_ref.py): small inputs at which the tile kernel, the
slice and the selection can go wrong.  Shared by the host emulation (tests/test_dist_emulation.py) and the GPU tests
(tests/test_gpu_dist.py).  Every case is a few seconds of NumPy at most."""
import collections
import functools

import numpy as np

NO_GROUP = 0xFFFFFFFF
Case = collections.namedtuple("Case", "name q r n qgroup rgroup")   # q, r: uint8 [n, P]; groups: uint32 arrays or None

EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
K_STEPS = (1, 63, 64, 65, 127, 129, 4095, 4097)
EXTREME_PIXELS = (262144, 131769)   # 512^2 and 363^2
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


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, built once; the arrays are read-only."""
    cases = _pad() + _tile_edges() + _k_steps() + _structured() + _extremes() + _ties() + _groups() + _n_values()
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
    return m, idx, d2
