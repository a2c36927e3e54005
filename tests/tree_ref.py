"""The rule of `tree` ("`tree`: the rule"; include/vkimg.h, vk_tree_nj_device), stated twice: as plain
Python loops, and in NumPy with a vectorised argmin.  All arithmetic is IEEE double, one operation at a time in the order
written (Python floats and NumPy's elementwise operations never fuse a multiply with an add); the device equals both bit
for bit.  Beside the rule: a Newick writer and reader, the splits of a join record, the per-block pair counts as a loop,
and the replicate chooser (the same generator as varkoder_amd/tree.py, written out again so that either can be held
against the other).

A record of n leaves has 2 (n - 3) + 3 entries: step t joined slots nodes[2t] < nodes[2t + 1] with branch lengths
lengths[2t], lengths[2t + 1], the new node taking the lower slot; the last three entries are the slots a < b < c still
active and their lengths."""
import math
import re

import numpy as np

BAD_VALUE = 1
MAX_ENTRY = 1e100
PARTIALS = 256
BLOCKS = 64
MASK = (1 << 64) - 1
GOLDEN, C1, C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def record_len(n):
    return 2 * (n - 3) + 3


# ---------------------------------------------------------------------------------------------------- the rule, as loops --

def valid_loop(D):
    n = len(D)
    for i in range(n):
        for j in range(n):
            v = float(D[i][j])
            if not math.isfinite(v) or not v >= 0.0 or not v <= MAX_ENTRY:
                return False
            if np.float64(D[i][j]).tobytes() != np.float64(D[j][i]).tobytes():
                return False
        if not float(D[i][i]) == 0.0:
            return False
    return True


def fold(p):
    """p[t] += p[t + s] for s = 128, 64, .., 1; the sum is p[0]."""
    s = PARTIALS // 2
    while s:
        for t in range(s):
            p[t] = p[t] + p[t + s]
        s //= 2
    return p[0]


def row_sum_loop(D, i, active):
    p = [0.0] * PARTIALS
    for k in range(len(active)):
        if active[k] and k != i:
            p[k % PARTIALS] = p[k % PARTIALS] + D[i][k]
    return fold(p)


def nj_loop(D):
    """(status, nodes, lengths) of one matrix (anything that indexes as [i][j], n >= 3)."""
    n = len(D)
    L = record_len(n)
    if not valid_loop(D):
        return BAD_VALUE, [0] * L, [0.0] * L
    D = [[float(D[i][j]) for j in range(n)] for i in range(n)]
    active = [True] * n
    R = [row_sum_loop(D, i, active) for i in range(n)]
    nodes, lengths = [], []
    m = n
    while m > 3:
        m2 = float(m - 2)
        best = None
        for i in range(n):
            if not active[i]:
                continue
            for j in range(i + 1, n):
                if not active[j]:
                    continue
                q = (m2 * D[i][j] - R[i]) - R[j]
                if best is None or q < best[0]:   # (rising i, then rising j: the first of equal values stays)
                    best = (q, i, j)
        _, i, j = best
        dij = D[i][j]
        li = 0.5 * dij + (R[i] - R[j]) / (2.0 * m2)
        lj = dij - li
        nodes += [i, j]
        lengths += [li, lj]
        for k in range(n):
            if not active[k] or k == i or k == j:
                continue
            du = 0.5 * ((D[i][k] + D[j][k]) - dij)
            R[k] = ((R[k] - D[i][k]) - D[j][k]) + du
            D[i][k] = du
            D[k][i] = du
        active[j] = False
        R[i] = row_sum_loop(D, i, active)
        m -= 1
    a, b, c = [k for k in range(n) if active[k]]
    nodes += [a, b, c]
    lengths += [0.5 * ((D[a][b] + D[a][c]) - D[b][c]), 0.5 * ((D[a][b] + D[b][c]) - D[a][c]),
                0.5 * ((D[a][c] + D[b][c]) - D[a][b])]
    return 0, nodes, lengths


# --------------------------------------------------------------------------------------------------- the rule, in NumPy --

def valid_np(D):
    D = np.asarray(D, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(D).all() and (D >= 0.0).all() and (D <= MAX_ENTRY).all() and (np.diagonal(D) == 0.0).all()
    return bool(ok and np.array_equal(D.view(np.uint64), D.T.view(np.uint64)))


def row_sums_np(rows, skip):
    """The 256-partial sums of rows [r, n] in which the entries to skip have been set to +0.0 (adding +0.0 to a partial
    that began at +0.0 never changes a bit of it: such a partial is never -0.0)."""
    r, n = rows.shape
    pad = -n % PARTIALS
    x = np.where(skip, 0.0, rows)
    x = np.concatenate([x, np.zeros((r, pad))], axis=1).reshape(r, -1, PARTIALS)
    p = np.zeros((r, PARTIALS))
    for c in range(x.shape[1]):
        p = p + x[:, c, :]
    s = PARTIALS // 2
    while s:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0].copy()


def nj_np(D, steps=None):
    """(status, nodes uint32[L], lengths float64[L]); steps: stop after so many joins (timing a sample of them)."""
    D = np.array(D, dtype=np.float64)
    n = D.shape[0]
    L = record_len(n)
    if not valid_np(D):
        return BAD_VALUE, np.zeros(L, dtype=np.uint32), np.zeros(L)
    active = np.ones(n, dtype=bool)
    R = row_sums_np(D, np.eye(n, dtype=bool))
    nodes, lengths = np.zeros(L, dtype=np.uint32), np.zeros(L)
    m, t = n, 0
    while m > 3 and (steps is None or t < steps):
        act = np.flatnonzero(active)
        m2 = np.float64(m - 2)
        sub = D[np.ix_(act, act)]
        Q = (m2 * sub - R[act][:, None]) - R[act][None, :]
        Q[np.tril_indices(m)] = np.inf
        at = int(np.argmin(Q))            # (the first of equal values in row-major order: the smaller i, then the smaller j)
        i, j = int(act[at // m]), int(act[at % m])
        dij = D[i, j]
        li = 0.5 * dij + (R[i] - R[j]) / (2.0 * m2)
        nodes[2 * t], nodes[2 * t + 1] = i, j
        lengths[2 * t], lengths[2 * t + 1] = li, dij - li
        ks = act[(act != i) & (act != j)]
        du = 0.5 * ((D[i, ks] + D[j, ks]) - dij)
        R[ks] = ((R[ks] - D[i, ks]) - D[j, ks]) + du
        D[i, ks] = du
        D[ks, i] = du
        active[j] = False
        skip = ~active
        skip[i] = True
        R[i] = row_sums_np(D[i:i + 1], skip[None, :])[0]
        m -= 1
        t += 1
    if m == 3:
        a, b, c = (int(x) for x in np.flatnonzero(active))
        nodes[-3:] = a, b, c
        lengths[-3:] = (0.5 * ((D[a, b] + D[a, c]) - D[b, c]), 0.5 * ((D[a, b] + D[b, c]) - D[a, c]),
                        0.5 * ((D[a, c] + D[b, c]) - D[a, b]))
    return 0, nodes, lengths


def nj_batch(D):
    """A call's worth: D [ntrees, n, n] -> (status uint32[ntrees], nodes uint32[ntrees, L], lengths float64[ntrees, L])."""
    out = [nj_np(d) for d in D]
    return (np.array([o[0] for o in out], dtype=np.uint32), np.array([o[1] for o in out], dtype=np.uint32).reshape(len(out), -1),
            np.array([o[2] for o in out], dtype=np.float64).reshape(len(out), -1))


# ------------------------------------------------------------------------------------------ trees, Newick and the splits --

def children(n, nodes):
    """The tree of a record: (top, kids) with kids[node] = ((child, at), (child, at)) for the node made by step t
    (numbered n + t), leaves 0 .. n - 1, `at` the index of the branch's length in the record; top: the three
    (node, at) of the trifurcation."""
    slot = list(range(n))
    kids = {}
    for t in range(n - 3):
        i, j = int(nodes[2 * t]), int(nodes[2 * t + 1])
        kids[n + t] = ((slot[i], 2 * t), (slot[j], 2 * t + 1))
        slot[i] = n + t
    base = 2 * (n - 3)
    return [(slot[int(nodes[base + x])], base + x) for x in range(3)], kids


def splits(n, nodes):
    """The bipartition under every step's node, as the frozenset of the leaves on the side without leaf 0, in step order."""
    _, kids = children(n, nodes)
    under, out = {}, []
    for t in range(n - 3):
        leaves = frozenset()
        for child, _ in kids[n + t]:
            leaves |= under[child] if child >= n else frozenset([child])
        under[n + t] = leaves
        out.append(frozenset(range(n)) - leaves if 0 in leaves else leaves)
    return out


def no_negative(n, lengths):
    """Kuhner and Felsenstein (1994): of a joined pair, a negative length becomes 0 and the sibling takes it, so that the
    path through the pair keeps its length; the closing three stay as computed."""
    out = [float(x) for x in lengths]
    for t in range(n - 3):
        li, lj = out[2 * t], out[2 * t + 1]
        if li < 0.0:
            out[2 * t], out[2 * t + 1] = 0.0, lj + li
        elif lj < 0.0:
            out[2 * t], out[2 * t + 1] = li + lj, 0.0
    return out


PLAIN = re.compile(r"[A-Za-z0-9.+-]+\Z")


def quote(name):
    return name if PLAIN.match(name) else "'" + name.replace("'", "''") + "'"


def newick(names, nodes, lengths, labels=None):
    """Unrooted Newick with a trifurcation at the top; labels: {step: text} for the internal nodes."""
    n = len(names)
    top, kids = children(n, nodes)

    def text(node, at):
        if node < n:
            return quote(names[node]) + ":" + repr(float(lengths[at]))
        inner = ",".join(text(c, a) for c, a in kids[node])
        return "(" + inner + ")" + (labels or {}).get(node - n, "") + ":" + repr(float(lengths[at]))
    return "(" + ",".join(text(c, a) for c, a in top) + ");\n"


def read_newick(s):
    """A Newick string as nested (label, length, [children]) -- quoted labels, lengths and internal labels understood."""
    pos = 0

    def label():
        nonlocal pos
        if pos < len(s) and s[pos] == "'":
            out = ""
            pos += 1
            while True:
                if s[pos] == "'":
                    if s[pos + 1:pos + 2] == "'":
                        out += "'"
                        pos += 2
                        continue
                    pos += 1
                    return out
                out += s[pos]
                pos += 1
        start = pos
        while pos < len(s) and s[pos] not in "():,;":
            pos += 1
        return s[start:pos]

    def node():
        nonlocal pos
        kids = []
        if s[pos] == "(":
            pos += 1
            kids.append(node())
            while s[pos] == ",":
                pos += 1
                kids.append(node())
            assert s[pos] == ")"
            pos += 1
        name = label()
        length = None
        if pos < len(s) and s[pos] == ":":
            pos += 1
            start = pos
            while s[pos] not in "(),;":
                pos += 1
            length = float(s[start:pos])
        return name, length, kids
    tree = node()
    assert s[pos] == ";"
    return tree


# ------------------------------------------------------------------------------------- the blocks and the replicates --

def pair_blocks_loop(sa, sb, s):
    """(shared[64], seen[64]) of two sketches made with the same s: among the seen = min(s, |Sa u Sb|) smallest values of
    the union, how many have h & 63 == b, and how many of those lie in both."""
    a, b = set(int(x) for x in sa), set(int(x) for x in sb)
    union = sorted(a | b)
    shared, seen = [0] * BLOCKS, [0] * BLOCKS
    for v in union[:min(s, len(union))]:
        seen[v & 63] += 1
        if v in a and v in b:
            shared[v & 63] += 1
    return shared, seen


def mix(z):
    z = ((z ^ (z >> 30)) * C1) & MASK
    z = ((z ^ (z >> 27)) * C2) & MASK
    return z ^ (z >> 31)


def kept_blocks(seed, r):
    """The 32 blocks that replicate r keeps: splitmix64 from the state mix(seed + GOLDEN) ^ r, one output per swap of a
    Fisher-Yates shuffle of 0 .. 63 from the top down (j = output mod (i + 1)); the first 32 of the result, ascending."""
    state = mix((seed + GOLDEN) & MASK) ^ (r & MASK)
    order = list(range(BLOCKS))
    for i in range(BLOCKS - 1, 0, -1):
        state = (state + GOLDEN) & MASK
        j = mix(state) % (i + 1)
        order[i], order[j] = order[j], order[i]
    return sorted(order[:BLOCKS // 2])


def support(n, main_nodes, replicate_nodes):
    """How many of the replicate records contain each split of the main record (in step order)."""
    have = [set(splits(n, nodes)) for nodes in replicate_nodes]
    return [sum(1 for h in have if sp in h) for sp in splits(n, main_nodes)]
