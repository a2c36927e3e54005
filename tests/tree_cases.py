"""The matrices of the `tree` tests: additive trees (whose topology and edge lengths neighbour joining must return), noisy
and arbitrary symmetric matrices (where only the rule decides), the tie matrices, and the invalid ones.

The tie matrices: `ones` (every pair ties at every step: at 513 and 600 leaves across every tile, strip and workgroup of
the search), `three_identical`, and `exact_cherries`: an additive tree of even integer branch lengths, so that every R,
Q, Du and length of the run is an integer that a double holds exactly and equal values are equal bit for bit, in which
chosen pairs of slots -- in different column tiles and row strips of the search -- are cherries of one and the same
smallest Q: the smaller (i, j) must win whichever workgroup found it."""
import random

import numpy as np


def random_tree(rng, n):
    """A random unrooted binary tree of n >= 3 leaves: edges [(u, v, length)], leaves 0 .. n - 1, inner nodes from n."""
    edges = [(0, n, rng.uniform(0.01, 1.0)), (1, n, rng.uniform(0.01, 1.0)), (2, n, rng.uniform(0.01, 1.0))]
    inner = n + 1
    for leaf in range(3, n):
        u, v, w = edges.pop(rng.randrange(len(edges)))
        cut = rng.uniform(0.2, 0.8) * w
        edges += [(u, inner, cut), (inner, v, w - cut), (leaf, inner, rng.uniform(0.01, 1.0))]
        inner += 1
    return edges


def tree_distances(n, edges):
    """The path lengths between the leaves of a tree."""
    nodes = 1 + max(max(u, v) for u, v, _ in edges)
    near = [[] for _ in range(nodes)]
    for u, v, w in edges:
        near[u].append((v, w))
        near[v].append((u, w))
    D = np.zeros((n, n))
    for a in range(n):
        dist = {a: 0.0}
        todo = [a]
        while todo:
            u = todo.pop()
            for v, w in near[u]:
                if v not in dist:
                    dist[v] = dist[u] + w
                    todo.append(v)
        for b in range(n):
            D[a, b] = dist[b]
    return np.maximum(D, D.T)   # (bit-for-bit symmetric: the two walks add in different orders)


def tree_splits(n, edges):
    """{split: edge length} of the inner edges, a split the frozenset of the leaves on the side without leaf 0."""
    nodes = 1 + max(max(u, v) for u, v, _ in edges)
    near = [[] for _ in range(nodes)]
    for u, v, _ in edges:
        near[u].append(v)
        near[v].append(u)
    out = {}
    for u, v, w in edges:
        if u < n or v < n:
            continue
        side, todo = {u}, [u]
        while todo:
            x = todo.pop()
            for y in near[x]:
                if y != v and y not in side:
                    side.add(y)
                    todo.append(y)
        leaves = frozenset(x for x in side if x < n)
        out[frozenset(range(n)) - leaves if 0 in leaves else leaves] = w
    return out


def leaf_edges(n, edges):
    return {min(u, v): w for u, v, w in edges if min(u, v) < n}


def additive(n, seed):
    """(D, edges) of a random tree."""
    edges = random_tree(random.Random(seed), n)
    return tree_distances(n, edges), edges


def noisy(n, seed):
    """An additive matrix with every pair's distance scaled by up to 10 %: no tree fits, the rule alone decides."""
    D, _ = additive(n, seed)
    rng = np.random.default_rng(seed)
    f = np.triu(rng.uniform(0.9, 1.1, (n, n)), 1)
    return D * (f + f.T)


def arbitrary(n, seed):
    """Symmetric, non-negative, otherwise anything (no triangle inequality: lengths and updated distances go negative)."""
    rng = np.random.default_rng(seed)
    U = np.triu(rng.uniform(0.0, 1.0, (n, n)) ** 3, 1)
    return U + U.T


def ones(n):
    return np.ones((n, n)) - np.eye(n)


def exact_cherries(n, pairs, seed):
    """Slots a < b of every one of `pairs` are a cherry with leaf lengths 2 and 4 whose parent hangs by one long edge from
    a hub; the other leaves form a random tree of edge lengths 2 .. 8 around the hub.  The cherries are alike (the same
    lengths, the same distances to every other leaf and to each other's leaves): their Q is the same integer, and the
    long edge makes it the smallest of the matrix.  Asserted here for step 0, in NumPy."""
    pairs = [tuple(p) for p in pairs]
    special = [s for p in pairs for s in p]
    assert all(0 <= a < b < n for a, b in pairs) and len(set(special)) == len(special) and n - len(special) >= 3
    rng = random.Random(seed)
    rest = n - len(special)                      # leaves 0 .. rest - 1 of the random tree; leaf `rest` becomes the hub
    length = lambda: 2.0 * rng.randint(1, 4)     # noqa: E731
    edges = [(0, rest + 1, length()), (1, rest + 1, length()), (2, rest + 1, length())]
    inner = rest + 2
    for leaf in range(3, rest + 1):
        u, v, w = edges.pop(rng.randrange(len(edges)))
        edges += [(u, inner, w), (inner, v, length()), (leaf, inner, length())]
        inner += 1
    hub = rest
    depth = tree_distances(rest + 1, edges)[hub].max()
    far = 2.0 * (int(depth) // 2 + 1)            # the long edge: past every leaf's distance from the hub
    # relabel: the tree's leaves keep their order in the slots the pairs leave free; nodes from n on are inner
    free = [s for s in range(n) if s not in set(special)]
    name = {leaf: free[leaf] for leaf in range(rest)}
    name.update({node: n + node for node in range(rest, inner)})
    edges = [(name[u], name[v], w) for u, v, w in edges]
    top = n + inner
    for a, b in pairs:
        edges += [(a, top, 2.0), (b, top, 4.0), (top, name[hub], far)]
        top += 1
    D = tree_distances(n, edges)
    assert np.array_equal(D, D.T) and np.array_equal(D, 2.0 * np.round(D / 2.0)) and D.max() < 2.0 ** 20   # even integers
    R = D.sum(axis=1)                            # (integers far below 2^53: exact in any order)
    Q = (float(n - 2) * D - R[:, None]) - R[None, :]
    Q[np.tril_indices(n)] = np.inf
    least = Q.min()
    assert all(Q[a, b].tobytes() == least.tobytes() for a, b in pairs), "the cherries do not share the smallest Q"
    assert sorted(zip(*(x.tolist() for x in np.nonzero(Q == least)))) == sorted(pairs), "another pair ties with the cherries"
    return D


def three_identical(n=7, seed=5):
    """Samples 1, 3 and 4 identical (distance 0 between them, equal rows otherwise)."""
    D = noisy(n, seed)
    for k in (3, 4):
        D[k, :] = D[1, :]
        D[:, k] = D[:, 1]
    for a in (1, 3, 4):
        for b in (1, 3, 4):
            D[a, b] = 0.0
    np.fill_diagonal(D, 0.0)
    return D


def invalid(kind, n=9, seed=2):
    D = noisy(n, seed)
    if kind == "nan":
        D[2, 5] = D[5, 2] = np.nan
    elif kind == "inf":
        D[2, 5] = D[5, 2] = np.inf
    elif kind == "negative":
        D[1, 7] = D[7, 1] = -1e-9
    elif kind == "asymmetric":
        D[3, 4] = np.nextafter(D[4, 3], 2.0)
    elif kind == "diagonal":
        D[6, 6] = 1e-300
    elif kind == "too_large":
        D[0, 8] = D[8, 0] = 2e100
    else:
        raise ValueError(kind)
    return D


INVALID = ("nan", "inf", "negative", "asymmetric", "diagonal", "too_large")
