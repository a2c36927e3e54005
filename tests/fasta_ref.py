"""The counting rule of `--from-fasta` in plain Python ("--from-fasta"): FASTA bytes to the FASTQ bytes
that hold one read per record, and from there oracle.count_fastq -- so that the pinned oracle defines every byte class.
brute_count is a second statement of the same rule that shares no code with the first (no line splitting, no FASTQ, no
oracle): a byte-at-a-time walk.  The GPU (vk_count_fasta_device) must equal count() exactly."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VK_ST_BAD_START = 1


def records(data):
    """The records of a FASTA byte string: the joined bytes of each, in order (a record without sequence gives b"").
    Lines end at \\n; a \\r directly before it, or as the sample's last byte, belongs to the line end."""
    data = bytes(data)
    lines = data.split(b"\n")
    last_open = not data.endswith(b"\n")
    out = []
    for i, ln in enumerate(lines):
        ended = i < len(lines) - 1
        if ln.endswith(b"\r") and (ended or last_open):   # (the piece behind the last \n is the sample's end)
            ln = ln[:-1]
        if ln.startswith(b">"):
            out.append(bytearray())
        elif ln:
            if not out:       # text before any header: the sample has a bad start, its records are not used
                out.append(bytearray())
            out[-1] += ln
    return [bytes(r) for r in out]


def status(data):
    return VK_ST_BAD_START if len(data) and bytes(data[:1]) != b">" else 0


def bases(data):
    """Sequence bytes of the sample: the joined bytes of its records, every class."""
    return sum(len(r) for r in records(data))


def to_fastq(data):
    """The FASTQ text with one read per record that has sequence bytes, in order."""
    out = bytearray()
    for i, r in enumerate(records(data)):
        if r:
            out += b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n"
    return bytes(out)


def count(data, k):
    """(hist uint32[4^k], status, bases) of a FASTA sample; one with a bad start is not read: zeros."""
    from oracle import oracle
    st = status(data)
    if st:
        return np.zeros(4 ** k, dtype=np.uint32), st, 0
    fq = to_fastq(data)
    fwd, _, ost = oracle.count_fastq(fq, k)
    assert ost == 0
    return fwd, 0, bases(data)


_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def brute_stretches(data):
    """(the unbroken stretches of bases as arrays of codes, bases): one pass over the bytes with the state a reader of
    the rule would keep."""
    data = bytes(data)
    n = len(data)
    nb = 0
    out, cur = [], []      # cur: the bases of the current unbroken stretch
    line_start, header = True, False
    for i, b in enumerate(data):
        if line_start:
            header = b == 62
            line_start = False
            if header and cur:
                out.append(cur)
                cur = []
        if b == 10:
            line_start = True
            continue
        if header:
            continue
        if b == 13 and (i + 1 == n or data[i + 1] == 10):
            continue
        nb += 1
        c = _CODE.get(b)
        if c is None:
            if cur:
                out.append(cur)
                cur = []
            continue
        cur.append(c)
    if cur:
        out.append(cur)
    return [np.array(x, dtype=np.int64) for x in out], nb


def brute_count(data, k, walked=None):
    """(hist uint64[4^k], bases): every window of k codes inside a stretch of brute_stretches (walked: its result)."""
    stretches, nb = walked if walked is not None else brute_stretches(data)
    hist = np.zeros(4 ** k, dtype=np.uint64)
    for a in stretches:
        if len(a) < k:
            continue
        v = np.zeros(len(a) - k + 1, dtype=np.int64)
        for j in range(k):
            v = v * 4 + a[j:len(a) - k + 1 + j]
        np.add.at(hist, v, 1)
    return hist, nb
