"""The rule of `compare` ("`compare`: the rule") in NumPy int64: the matrix of exact squared Euclidean
distances, the neighbours by (d2, j) among the eligible references, the fill.  Written from the rule's text, with no
look at the kernels: differences of pixels squared and summed, a stable sort."""
import numpy as np

NO_GROUP = 0xFFFFFFFF
NO_IDX = np.uint32(0xFFFFFFFF)
NO_D2 = np.uint64(0xFFFFFFFFFFFFFFFF)


def matrix(q, r):
    """d2 uint64 [nq, nr] of uint8 arrays [nq, P] and [nr, P]."""
    q = np.asarray(q).reshape(len(q), -1).astype(np.int64)
    r = np.asarray(r).reshape(len(r), -1).astype(np.int64)
    out = np.empty((len(q), len(r)), dtype=np.int64)
    for i in range(len(q)):
        d = r - q[i]
        out[i] = np.einsum("jp,jp->j", d, d)
    return out.astype(np.uint64)


def neighbours(d2, n, qgroup=None, rgroup=None):
    """(idx uint32 [nq, n], d2 uint64 [nq, n]) of a matrix."""
    nq, nr = d2.shape
    idx = np.full((nq, n), NO_IDX, dtype=np.uint32)
    out = np.full((nq, n), NO_D2, dtype=np.uint64)
    for i in range(nq):
        ok = np.ones(nr, dtype=bool)
        if qgroup is not None and int(qgroup[i]) != NO_GROUP:
            ok = np.asarray(rgroup, dtype=np.uint64) != np.uint64(qgroup[i])
        js = np.flatnonzero(ok)
        order = js[np.argsort(d2[i, js], kind="stable")][:n]   # (js ascends: equal distances keep the lower j first)
        idx[i, :len(order)] = order
        out[i, :len(order)] = d2[i, order]
    return idx, out
