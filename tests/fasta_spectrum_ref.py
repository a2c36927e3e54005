"""The rule of `--genome-spectrum` in plain Python ("`--genome-spectrum`: the rule"), stated twice, and the
assembly's estimates.  vk_spectrum_fasta_device must equal the rule exactly.

A sample is one FASTA text.  Its lines, header lines and records are `--from-fasta`'s (tests/fasta_ref.py): a line ends at
\\n, a \\r directly before it (or as the text's last byte) belongs to the line end, a line that begins with '>' is a header
and holds no sequence, the other lines join into the current record, empty lines vanish.  Bases, windows and keys are the
screen's (tests/screen_ref.py): ACGT of either case is coded 0 1 2 3, every other sequence byte and every record boundary
breaks the sequence, every window of K (16..31) unbroken bases -- across line ends -- gives a key, the smaller of the window
and its reverse complement read as 2K-bit integers, first base most significant.  A key is TAKEN when (mix(key) >> 32) %
every == 0 (tests/spectrum_ref.py's mix); every occurrence of a taken key counts.

A row is spectrum_ref.NSTAT integers: records (header lines), bases (the records' joined bytes, every class), windows, taken
windows, distinct (taken keys), hist[0..255] with hist[c - 1] = distinct taken keys of multiplicity c (hist[255]: 256 and
more).  A multiplicity is a copy number here, not a depth.  A non-empty text that does not begin with '>' has status
VK_ST_BAD_START, a sample whose distinct taken keys exceed its table's slots VK_SPEC_TABLE_FULL; either gets an all-zero row.
An empty text has status 0 and a zero row.

First statement (counts_strings): the records as fasta_ref.records joins them, every window a Python bytes string, its key
by int(., 4) of it and of its reverse complement.  Second statement (counts_numpy): the text as one NumPy array, no line is
split: header bytes by the cumulative count of line ends, codes through a table, keys K shifts at a time, multiplicities by
np.unique.  They share no code but mix; tests/test_fasta_spectrum_rules.py holds them to each other and to the screen's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_ref  # noqa: E402
import spectrum_ref  # noqa: E402

NSTAT, HIST_AT, BINS = spectrum_ref.NSTAT, spectrum_ref.HIST_AT, spectrum_ref.BINS
RECORDS, BASES, WINDOWS, TAKEN, DISTINCT = range(5)
VK_ST_BAD_START, VK_SPEC_TABLE_FULL = 1, 32
MIN_SLOTS = 1024


def slots_for(length, every=1):
    """The table the engine gives an assembly of `length` bytes."""
    want = max(MIN_SLOTS, 2 * -(-length // every))
    return 1 << (want - 1).bit_length()


def row_of(records, bases, windows, counts):
    return spectrum_ref.row_of(records, bases, windows, counts)


def _finish(data, records, bases, windows, counts, slots):
    if len(data) and bytes(data[:1]) != b">":
        return [0] * NSTAT, VK_ST_BAD_START, {}
    if slots is not None and len(counts) > slots:
        return [0] * NSTAT, VK_SPEC_TABLE_FULL, {}
    return row_of(records, bases, windows, counts), 0, counts


# ------------------------------------------------------------ first statement --

_DIGITS = bytes.maketrans(b"ACGT", b"0123")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def counts_strings(data, k, every=1):
    """(records, bases, windows, {taken key: multiplicity}) of a text that begins with '>' (or is empty)."""
    recs = fasta_ref.records(data)
    windows, counts = 0, {}
    for rec in recs:
        up = rec.upper()
        for i in range(len(up) - k + 1):
            w = up[i:i + k]
            if w.strip(b"ACGT"):
                continue
            windows += 1
            key = min(int(w.translate(_DIGITS), 4), int(w.translate(_COMP)[::-1].translate(_DIGITS), 4))
            if spectrum_ref.taken(key, every):
                counts[key] = counts.get(key, 0) + 1
    return len(recs), sum(len(r) for r in recs), windows, counts


def spectrum_strings(data, k, every=1, slots=None):
    """(row, status, {taken key: multiplicity})."""
    data = bytes(data)
    if len(data) and data[:1] != b">":
        return [0] * NSTAT, VK_ST_BAD_START, {}
    return _finish(data, *counts_strings(data, k, every), slots)


# ----------------------------------------------------------- second statement --

_LUT = np.full(256, 4, dtype=np.uint64)
for _b, _c in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _LUT[_b] = _c


def counts_numpy(data, k, every=1):
    """(records, bases, windows, sorted taken keys uint64, their multiplicities)."""
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(b)
    none = np.zeros(0, dtype=np.uint64)
    if n == 0:
        return 0, 0, 0, none, none.astype(np.int64)
    nl = b == 10
    start = np.concatenate(([True], nl[:-1]))                 # the byte starts a line
    line = np.cumsum(start) - 1                                # the byte's line
    header = (b[start] == 62)[line]                            # the byte lies in a header line
    nxt_nl = np.concatenate((nl[1:], [True]))                  # the next byte is a line end, or there is none
    line_end_cr = (b == 13) & nxt_nl
    seq = ~nl & ~header & ~line_end_cr                         # a sequence byte, whatever its class
    records = int((start & (b == 62)).sum())
    bases = int(seq.sum())
    # the codes of the sequence bytes, one break for every header byte (a header line has one at least)
    keep = seq | header
    codes = np.where(header, np.uint64(4), _LUT[b])[keep]
    m = len(codes) - k + 1
    if m <= 0:
        return records, bases, 0, none, none.astype(np.int64)
    bad = np.concatenate(([0], np.cumsum(codes > 3)))
    ok = (bad[k:] - bad[:-k]) == 0
    low = codes & np.uint64(3)
    fw = np.zeros(m, dtype=np.uint64)
    rc = np.zeros(m, dtype=np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | low[j:j + m]
        rc = (rc << np.uint64(2)) | (np.uint64(3) - low[k - 1 - j:k - 1 - j + m])
    keys = np.minimum(fw, rc)[ok]
    sel = keys[(spectrum_ref.mix_np(keys) >> np.uint64(32)) % np.uint64(every) == 0] if every > 1 else keys
    uniq, mult = np.unique(sel, return_counts=True)
    return records, bases, len(keys), uniq, mult.astype(np.int64)


def spectrum_numpy(data, k, every=1, slots=None):
    """(row as uint64[NSTAT], status, sorted taken keys, their multiplicities)."""
    row = np.zeros(NSTAT, dtype=np.uint64)
    none = np.zeros(0, dtype=np.uint64)
    data = bytes(data)
    if len(data) and data[:1] != b">":
        return row, VK_ST_BAD_START, none, none.astype(np.int64)
    records, bases, windows, uniq, mult = counts_numpy(data, k, every)
    if slots is not None and len(uniq) > slots:
        return row, VK_SPEC_TABLE_FULL, none, none.astype(np.int64)
    row[RECORDS], row[BASES], row[WINDOWS] = records, bases, windows
    row[TAKEN], row[DISTINCT] = int(mult.sum()), len(uniq)
    if len(mult):
        row[HIST_AT:] = np.bincount(np.minimum(mult, BINS) - 1, minlength=BINS)
    return row, 0, uniq, mult


def table_numpy(data, k, every=1):
    """The counting table of a good sample as a pair (keys uint64 sorted, counts uint32): what sketch_ref takes."""
    _, _, _, uniq, mult = counts_numpy(data, k, every)
    return uniq, mult.astype(np.uint32)


# ------------------------------------------------------------------ estimates --

def assembly_estimate(row, k, every=1):
    """The estimates of an assembly's row, formula by formula."""
    taken, distinct, ones = int(row[TAKEN]), int(row[DISTINCT]), int(row[HIST_AT])
    return {"kmer_coverage": None, "base_coverage": None, "genome_kmers": every * distinct, "error_kmers": None,
            "error_rate": None, "high_copy_fraction": (taken - ones) / taken if taken else None,
            "singleton_fraction": ones / distinct if distinct else None, "seen_fraction": 1.0, "reason": "assembly"}
