"""The rule of `--depth-filter` in plain Python ("`--depth-filter`: the rule"), stated twice.
vk_depth_device must equal the rule exactly: output bytes, lengths, rows and status.

A sample is a cleaned FASTQ text, framed as the screen frames it (tests/screen_ref.py).  Its table is its spectrum's
(tests/spectrum_ref.py): the multiplicity of every TAKEN key of the whole sample.  For one record: the depth c(w) of a
taken window is its key's multiplicity (0 when the table does not hold the key -- in a table counted from the same text
that does not happen, the emulation covers it); n is the number of taken windows; the record's depth m is 0 when n == 0,
else the element at index (n - 1) // 2 of the sorted c(w); the record is kept when lo <= m <= hi, whole, byte for byte,
in input order.

A row is NSTAT = 261 integers: records in, records kept, sequence bases in, sequence bases kept, records with n == 0,
hist[0..255] with hist[min(m, 255)] counted over all records in.  A sample with a framing status, or whose table filled
(`slots` given and fewer than the distinct taken keys: VK_SPEC_TABLE_FULL), gets no text and an all-zero row.

First statement (depth_sort): record by record, screen_ref's rolling keys, a dict of multiplicities, sort and index.
Second statement (depth_count): the whole sample in NumPy arrays -- every window's key and record, multiplicities by
np.unique, the decision by the two counts #{c < lo} <= (n - 1) // 2 and #{c <= hi} > (n - 1) // 2 and the histogram's bin
by a cumulative sum over the record's 256 saturated bins.  They share the framing and spectrum_ref's key arithmetic only;
tests/test_depth_rules.py holds them to each other."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import screen_ref  # noqa: E402
import spectrum_ref as R  # noqa: E402

NSTAT, HIST_AT, BINS = 261, 5, 256
IN, KEPT, BASES_IN, BASES_KEPT, NO_WINDOWS = range(5)
OPEN = 2 ** 32 - 1
VK_SPEC_TABLE_FULL = R.VK_SPEC_TABLE_FULL


# ------------------------------------------------------------ first statement --

def record_depths(seq, counts, k, every):
    """The depths of a sequence line's taken windows, in window order."""
    codes = [screen_ref._CODE.get(b) for b in bytes(seq)]
    return [counts.get(key, 0) for _, key in screen_ref._roll(codes, k) if R.taken(key, every)]


def median(depths):
    return sorted(depths)[(len(depths) - 1) // 2] if depths else 0


def depth_sort(text, k, every, lo, hi, slots=None):
    """(kept text, row, status, kept flag per record) of a sample."""
    status, recs = screen_ref.split_records(text)
    if status:
        return b"", [0] * NSTAT, status, []
    counts = R.counts_loop(text, k, every)[3]
    if slots is not None and len(counts) > slots:
        return b"", [0] * NSTAT, VK_SPEC_TABLE_FULL, []
    out, row, flags = bytearray(), [0] * NSTAT, []
    for raw, seq in recs:
        d = record_depths(seq, counts, k, every)
        m = median(d)
        keep = lo <= m <= hi
        row[IN] += 1
        row[BASES_IN] += len(seq)
        row[NO_WINDOWS] += not d
        row[HIST_AT + min(m, BINS - 1)] += 1
        if keep:
            out += raw
            row[KEPT] += 1
            row[BASES_KEPT] += len(seq)
        flags.append(keep)
    return bytes(out), row, 0, flags


# ----------------------------------------------------------- second statement --

def windows_numpy(seqs, k):
    """(key, record) of every window of k unbroken bases of the sequence lines, as two arrays."""
    if not seqs:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    joined = np.frombuffer(b"\n".join(seqs), dtype=np.uint8)   # (a \n between two lines: no base, so no window spans them)
    codes = R._LUT[joined]
    rec = np.cumsum(joined == 10)
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    bad = np.concatenate(([0], np.cumsum(codes > 3)))
    ok = (bad[k:] - bad[:-k]) == 0
    low = codes & np.uint64(3)
    fw = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | low[j:j + n]
        rc = (rc << np.uint64(2)) | (np.uint64(3) - low[k - 1 - j:k - 1 - j + n])
    return np.minimum(fw, rc)[ok], rec[:n][ok].astype(np.int64)


def depth_count(text, k, every, lo, hi, slots=None):
    """(kept text, row as uint64[NSTAT], status, kept flag per record) of a sample."""
    row = np.zeros(NSTAT, dtype=np.uint64)
    status, recs = screen_ref.split_records(text)
    if status:
        return b"", row, status, []
    seqs = [seq for _, seq in recs]
    nrec = len(recs)
    keys, rec = windows_numpy(seqs, k)
    if every > 1:
        sel = (R.mix_np(keys) >> np.uint64(32)) % np.uint64(every) == 0
        keys, rec = keys[sel], rec[sel]
    uniq, inverse, mult = np.unique(keys, return_inverse=True, return_counts=True)
    if slots is not None and len(uniq) > slots:
        return b"", row, VK_SPEC_TABLE_FULL, []
    c = mult[inverse].astype(np.int64) if len(keys) else np.zeros(0, dtype=np.int64)
    n = np.bincount(rec, minlength=nrec)
    below = np.bincount(rec, weights=c < lo, minlength=nrec).astype(np.int64)
    atmost = np.bincount(rec, weights=c <= hi, minlength=nrec).astype(np.int64)
    rank = np.maximum(n - 1, 0) // 2
    keep = np.where(n > 0, (below <= rank) & (atmost > rank), lo == 0)
    # the median's bin: the first of the record's 256 saturated bins whose cumulative count passes the rank
    bins = np.bincount(rec * BINS + np.minimum(c, BINS - 1), minlength=nrec * BINS).reshape(nrec, BINS)
    mbin = np.where(n > 0, (np.cumsum(bins, axis=1) > rank[:, None]).argmax(axis=1), 0) if nrec else np.zeros(0, dtype=np.int64)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    row[IN], row[KEPT] = nrec, int(keep.sum())
    row[BASES_IN], row[BASES_KEPT] = int(lens.sum()), int(lens[keep].sum()) if nrec else 0
    row[NO_WINDOWS] = int((n == 0).sum())
    row[HIST_AT:] = np.bincount(mbin, minlength=BINS)
    out = b"".join(raw for (raw, _), f in zip(recs, keep) if f)
    return out, row, 0, [bool(f) for f in keep]
