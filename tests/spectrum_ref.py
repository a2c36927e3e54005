"""The rule of `--kmer-spectrum` in plain Python ("`--kmer-spectrum`: the rule"), stated twice, and the
estimator's formulas.  vk_spectrum_device must equal the rule exactly.

A sample is a cleaned FASTQ text, framed as the screen frames it (tests/screen_ref.py: VK_ST_*; a sample with a status
gets an all-zero row).  A read's windows come from its sequence line: a base is ACGT of either case, coded 0 1 2 3; a \\r
that ends the line is no part of it; every window of K (16..31) unbroken bases gives a key, the smaller of the window and
its reverse complement read as 2K-bit integers, first base most significant.  The quality line is not looked at.

A key is TAKEN when (mix(key) >> 32) % every == 0 (mix: splitmix64's finaliser).  Selection is by key: every occurrence of
a taken key counts.

A row is NSTAT = 261 integers: reads, bases (the sequence lines' bytes, every class, without the \\r), windows,
taken_windows, distinct (taken keys), hist[0..255] with hist[c - 1] = distinct taken keys of multiplicity c for c = 1..255
and hist[255] those of 256 and more.

First statement (spectrum_loop): one walk over the bytes with the line number a reader of the rule would keep, rolling
2-bit keys forward and reverse, a dict of multiplicities.  Second statement (spectrum_numpy): the records split by
screen_ref.split_records, every sequence line's codes in one NumPy array, the windows' keys built K shifts at a time, the
multiplicities by np.unique.  They share no code but the framing's status; tests/test_spectrum_rules.py holds them to each
other.

table_full(): what a table of `slots` slots does to a sample -- VK_SPEC_TABLE_FULL when the distinct taken keys exceed
the slots (with linear probing over the whole table a key finds a slot exactly while one is free)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_ref  # noqa: E402

NSTAT, HIST_AT, BINS = 261, 5, 256
READS, BASES, WINDOWS, TAKEN, DISTINCT = range(5)
VK_SPEC_TABLE_FULL = 32
K_MIN, K_MAX, MIN_SLOTS = 16, 31, 1024
M64 = (1 << 64) - 1
_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def mix(z):
    """splitmix64's finaliser on a Python integer."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def taken(key, every):
    return (mix(key) >> 32) % every == 0


def slots_for(length, every=1):
    """The table the engine gives a sample of `length` bytes."""
    want = max(MIN_SLOTS, 2 * -(-length // (2 * every)))
    return 1 << (want - 1).bit_length()


def row_of(reads, bases, windows, counts):
    """The row of a sample from its {taken key: multiplicity}."""
    row = [0] * NSTAT
    row[READS], row[BASES], row[WINDOWS] = reads, bases, windows
    row[TAKEN], row[DISTINCT] = sum(counts.values()), len(counts)
    for c in counts.values():
        row[HIST_AT + min(c, BINS) - 1] += 1
    return row


# ------------------------------------------------------------ first statement --

def counts_loop(text, k, every=1):
    """(reads, bases, windows, {taken key: multiplicity}) of a well-framed text, byte by byte."""
    text = bytes(text)
    n = len(text)
    mask = (1 << (2 * k)) - 1
    reads = bases = windows = 0
    counts = {}
    line = 0          # the line's number within its record
    fw = rc = run = 0
    for i, b in enumerate(text):
        if b == 10:
            line = (line + 1) % 4
            reads += line == 2   # (the sequence line has ended)
            fw = rc = run = 0
            continue
        if line != 1:
            continue
        if b == 13 and (i + 1 == n or text[i + 1] == 10):
            continue
        bases += 1
        c = _CODE.get(b)
        if c is None:
            run = 0
            continue
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * k - 2))
        run += 1
        if run >= k:
            windows += 1
            key = min(fw, rc)
            if taken(key, every):
                counts[key] = counts.get(key, 0) + 1
    return reads, bases, windows, counts


def spectrum_loop(text, k, every=1, slots=None):
    status = screen_ref.split_records(text)[0]
    if status:
        return [0] * NSTAT, status
    reads, bases, windows, counts = counts_loop(text, k, every)
    if slots is not None and len(counts) > slots:
        return [0] * NSTAT, VK_SPEC_TABLE_FULL
    return row_of(reads, bases, windows, counts), 0


# ----------------------------------------------------------- second statement --

_LUT = np.full(256, 4, dtype=np.uint64)
for _b, _c in _CODE.items():
    _LUT[_b] = _c


def mix_np(z):
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def keys_numpy(seqs, k):
    """The keys of every window of the sequence lines, as one uint64 array (in no particular order)."""
    if not seqs:
        return np.zeros(0, dtype=np.uint64)
    joined = b"\n".join(seqs)   # (a \n between two lines: no base, so no window spans them)
    codes = _LUT[np.frombuffer(joined, dtype=np.uint8)]
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    bad = np.concatenate(([0], np.cumsum(codes > 3)))
    ok = (bad[k:] - bad[:-k]) == 0
    low = codes & np.uint64(3)
    fw = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | low[j:j + n]
        rc = (rc << np.uint64(2)) | (np.uint64(3) - low[k - 1 - j:k - 1 - j + n])
    return np.minimum(fw, rc)[ok]


def spectrum_numpy(text, k, every=1, slots=None):
    """(row as uint64[NSTAT], status)."""
    row = np.zeros(NSTAT, dtype=np.uint64)
    status, recs = screen_ref.split_records(text)
    if status:
        return row, status
    seqs = [seq for _, seq in recs]
    keys = keys_numpy(seqs, k)
    sel = keys[(mix_np(keys) >> np.uint64(32)) % np.uint64(every) == 0] if every > 1 else keys
    _, mult = np.unique(sel, return_counts=True)
    if slots is not None and len(mult) > slots:
        return row, VK_SPEC_TABLE_FULL
    row[READS], row[BASES], row[WINDOWS] = len(seqs), sum(len(s) for s in seqs), len(keys)
    row[TAKEN], row[DISTINCT] = len(sel), len(mult)
    row[HIST_AT:] = np.bincount(np.minimum(mult, BINS) - 1, minlength=BINS)
    return row, 0


def taken_keys(text, k, every):
    """The sorted taken keys of a sample (second statement)."""
    keys = np.unique(keys_numpy([seq for _, seq in screen_ref.split_records(text)[1]], k))
    return keys[(mix_np(keys) >> np.uint64(32)) % np.uint64(every) == 0]


# ------------------------------------------------------------------ estimates --

def estimate(row, k, every=1):
    """The estimates of the rule from a row alone, formula by formula; values that need lambda are None with a reason."""
    h = lambda c: int(row[HIST_AT + c - 1])   # noqa: E731 -- h(c), c = 1..256 (256: the overflow bin)
    W, distinct, bases = int(row[TAKEN]), int(row[DISTINCT]), int(row[BASES])
    out = {"kmer_coverage": None, "base_coverage": None, "genome_kmers": None, "error_kmers": None, "error_rate": None,
           "high_copy_fraction": None, "singleton_fraction": h(1) / distinct if distinct else None, "support": 0,
           "reason": None}
    best, cstar = -1, 2
    for c in range(2, 255):
        if h(c) + h(c + 1) > best:
            best, cstar = h(c) + h(c + 1), c
    out["support"] = best
    if best < 1000 or h(cstar) == 0 or h(cstar + 1) == 0:   # (h(c* + 1) == 0: lambda would be 0 and G a division by 0)
        out["reason"] = "too few repeated k-mers"
        return out
    if cstar == 254 and h(255) + h(256) > h(254):
        out["reason"] = "coverage above the histogram"
        return out
    lam = (cstar + 1) * h(cstar + 1) / h(cstar)
    G = every * (distinct - h(1)) / (1 - math.exp(-lam) * (1 + lam))
    e1 = max(h(1) - (G / every) * lam * math.exp(-lam), 0.0)
    T = min(256, max(8, math.ceil(4 * lam)))
    below = sum(c * h(c) for c in range(1, min(T, 256)))
    out.update(kmer_coverage=lam, genome_kmers=G, error_kmers=e1, error_rate=1 - (1 - e1 / W) ** (1 / k),
               base_coverage=bases / G, high_copy_fraction=(W - below) / W)
    return out
