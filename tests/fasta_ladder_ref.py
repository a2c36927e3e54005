"""The rule of `image --from-fasta --fragments` in plain Python ("--from-fasta --fragments"), twice, with
no code shared between the two statements:

* count(): fasta_ref.records -> every record cut wherever the fragment number changes -> the pieces of taken fragments
  -> the FASTQ text with one read per piece -> oracle.count_fastq, so that the pinned oracle defines every byte class;
* brute_count(): a byte-at-a-time walk of the FASTA text (no line splitting, no records, no FASTQ, no oracle, its own
  restatement of the hash) that gives every base its ordinal; a step then keeps the windows of k bases that lie in one
  unbroken stretch and in one taken fragment.

J = the joined bytes of the sample's records, in order; ordinal q in [0, len(J)); fragment of q = (q + shift) div L;
fragment f is taken iff sample_hash(seed, f) < threshold.  Both also give `taken`, the ordinals in taken fragments.  The
GPU (vk_count_fasta_sampled_device) must equal count() exactly."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fasta_ref as FR  # noqa: E402
from ladder_emit_ref import sample_hash  # noqa: E402

ALL = 1 << 32
M64 = (1 << 64) - 1


def shift_of(seed, L):
    """The shift the host layer gives a step: sample_hash(seed, 2^64 - 1) mod L."""
    return sample_hash(seed, M64) % L


def pieces(data, L, seed, threshold, shift):
    """(the kept pieces of the sample's records, taken): each record cut where (q + shift) div L changes, the pieces of
    taken fragments kept."""
    out, taken, q = [], 0, 0
    for rec in FR.records(data):
        i = 0
        while i < len(rec):
            t = q + i + shift
            end = min(len(rec), i + L - t % L)
            if sample_hash(seed, t // L) < threshold:
                out.append(rec[i:end])
                taken += end - i
            i = end
        q += len(rec)
    return out, taken


def to_fastq(kept):
    return b"".join(b"@p%d\n" % i + p + b"\n+\n" + b"I" * len(p) + b"\n" for i, p in enumerate(kept))


def count(data, k, L, seed, threshold, shift):
    """(hist uint32[4^k], taken) of one step of a FASTA sample; one with a bad start gives zeros."""
    from oracle import oracle
    if FR.status(data):
        return np.zeros(4 ** k, dtype=np.uint32), 0
    kept, taken = pieces(data, L, seed, threshold, shift)
    fwd, _, ost = oracle.count_fastq(to_fastq(kept), k)
    assert ost == 0
    return fwd, taken


_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def brute_walk(data):
    """(code int64[B] with -1 for a non-base, record int64[B]): every sequence byte of the sample in ordinal order, and
    the number of header lines before it.  One pass over the bytes."""
    data = bytes(data)
    n = len(data)
    codes, recs = [], []
    line_start, header, nrec = True, False, 0
    for i, b in enumerate(data):
        if line_start:
            header = b == 62
            line_start = False
            nrec += header
        if b == 10:
            line_start = True
            continue
        if header or (b == 13 and (i + 1 == n or data[i + 1] == 10)):
            continue
        codes.append(_CODE.get(b, -1))
        recs.append(nrec)
    return np.array(codes, dtype=np.int64), np.array(recs, dtype=np.int64)


def hash_array(seed, f):
    """sample_hash over a uint64 array of fragment numbers."""
    m = np.uint64(0xFFFFFFFF)
    f = f.astype(np.uint64)
    h = (f ^ np.uint64(seed)) & m
    h = (h + (((f >> np.uint64(32)) * np.uint64(0x9E3779B1)) & m) + np.uint64(seed >> 32)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def brute_count(data, k, L, seed, threshold, shift, walked=None):
    """(hist uint64[4^k], taken) from brute_walk's arrays (walked: its result)."""
    hist = np.zeros(4 ** k, dtype=np.uint64)
    if len(data) and bytes(data[:1]) != b">":
        return hist, 0
    code, rec = walked if walked is not None else brute_walk(data)
    B = len(code)
    if B == 0:
        return hist, 0
    frag = (np.arange(B, dtype=np.uint64) + np.uint64(shift)) // np.uint64(L)
    take = hash_array(seed, frag) < np.uint64(threshold)
    taken = int(take.sum())
    if B >= k:
        nw = B - k + 1
        ok = take[:nw] & (frag[:nw] == frag[k - 1:]) & (rec[:nw] == rec[k - 1:])
        v = np.zeros(nw, dtype=np.int64)
        for j in range(k):
            c = code[j:nw + j]
            ok &= c >= 0
            v = v * 4 + np.maximum(c, 0)
        np.add.at(hist, v[ok], 1)
    return hist, taken


def steps(k):
    """Every step the tests list: L in {k, k + 1, 64, 150} x threshold in {0, 1, 2^31, 2^32 - 1, 2^32} x shift in
    {0, 1, L - 1, 2^32 - 70, 2^40 + 3} x two seeds, as (L, seed, threshold, shift)."""
    return [(L, seed, thr, shift)
            for L in (k, k + 1, 64, 150)
            for thr in (0, 1, 1 << 31, ALL - 1, ALL)
            for shift in (0, 1, L - 1, ALL - 70, (1 << 40) + 3)
            for seed in (7, 0x9E3779B97F4A7C15)]


@functools.lru_cache(maxsize=None)
def thinned(k, L, ncases, per_case):
    """per_case steps of steps(k) with fragment length L for each of ncases cases, dealt round-robin so that every
    combination of threshold, shift and seed comes up again and again across the cases: [[(L, seed, thr, shift)]]."""
    mine = [s for s in steps(k) if s[0] == L]
    stride = 7   # (coprime with the 50 steps of one L: consecutive cases get steps far apart in the product)
    return [[mine[(i * per_case + j) * stride % len(mine)] for j in range(per_case)] for i in range(ncases)]
