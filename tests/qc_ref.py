"""The rule of `--qc-report` in plain Python ("--qc-report: the rule"), stated twice.  vk_qc_device must
equal it exactly.

A stream is a FASTQ text with a record budget `records`: only its first `records` records count.  A line ends at \\n; the
text's last line may lack it; one \\r directly before the line's end is no part of the line.  The text holds
count(\\n) + (1 when its last byte is not \\n) lines, and a record is four of them: header, sequence, third line, quality.

Status.  VK_EM_BAD_RECORDS (alone) when the text holds fewer than 4 * records lines.  Otherwise VK_QC_BAD_FRAMING when the
header of one of the first `records` records does not begin with '@' or its third line does not begin with '+' (with or
without a name after it).  A stream with a status has an all-zero row.  What lies behind the budget is not looked at.

A record with ls != lq (the lengths of its sequence and quality lines) adds 1 to records and to ragged_records and nothing
else.  Every other record adds: records, bases (ls), gc_bases, other_bases, min_length / max_length (min_length is 0 in a
row without counted records), len_hist[min(ls, 1024)], qual_hist[q] per base, readq_hist[floor(sum q / ls)] when ls > 0,
and for every cycle c < 1024 cycle_base[c][class] and cycle_qsum[c][class] += q.  The class of a sequence byte: A C G T
of either case 0 1 2 3, every other byte 4.  The phred of a quality byte b: q = min(max(b - 33, 0), 93); a byte outside
33..126 also counts once in invalid_quality_bytes.

A row is NSTAT u64: 8 scalars (records, ragged_records, bases, gc_bases, other_bases, min_length, max_length,
invalid_quality_bytes), qual_hist[94], readq_hist[94], len_hist[1025], cycle_base[1024][5], cycle_qsum[1024][5].

First statement: row_loop -- the lines split with bytes.split, a loop over records and over their bytes.
Second statement: row_numpy -- newline positions, line bounds and every base of the stream as numpy index arrays, the
tables by bincount; shares no code with the first.  tests/test_qc_rules.py holds the two to each other."""
import numpy as np

VK_EM_BAD_RECORDS, VK_QC_BAD_FRAMING = 8, 16
CYCLES, PHREDS, LEN_BINS, CLASSES = 1024, 94, 1025, 5
RECORDS, RAGGED, BASES, GC, OTHER, MIN_LEN, MAX_LEN, INVALID = range(8)
QUAL_AT = 8
READQ_AT = QUAL_AT + PHREDS
LEN_AT = READQ_AT + PHREDS
BASE_AT = LEN_AT + LEN_BINS
QSUM_AT = BASE_AT + CYCLES * CLASSES
NSTAT = QSUM_AT + CYCLES * CLASSES

_CLASS = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def zero_row():
    return np.zeros(NSTAT, dtype=np.uint64)


def record_count(text):
    """The records a text holds when every one of them counts: its lines over four."""
    text = bytes(text)
    return (text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)) // 4


# ------------------------------------------------------------ first statement --

def _lines(text):
    parts = bytes(text).split(b"\n")
    if parts[-1] == b"":   # (the text ends with \n, or is empty)
        parts.pop()
    return parts


def _strip(line):
    return line[:-1] if line.endswith(b"\r") else line


def row_loop(text, records):
    """(row uint64[NSTAT], status) of one stream, byte by byte."""
    lines = _lines(text)
    if len(lines) < 4 * records:
        return zero_row(), VK_EM_BAD_RECORDS
    for r in range(records):
        if not lines[4 * r].startswith(b"@") or not lines[4 * r + 2].startswith(b"+"):
            return zero_row(), VK_QC_BAD_FRAMING
    row = [0] * NSTAT
    lengths = []
    for r in range(records):
        seq, qual = _strip(lines[4 * r + 1]), _strip(lines[4 * r + 3])
        row[RECORDS] += 1
        if len(seq) != len(qual):
            row[RAGGED] += 1
            continue
        ls = len(seq)
        lengths.append(ls)
        row[BASES] += ls
        row[LEN_AT + min(ls, LEN_BINS - 1)] += 1
        qsum = 0
        for c in range(ls):
            cls = _CLASS.get(seq[c], 4)
            b = qual[c]
            q = min(max(b - 33, 0), 93)
            if b < 33 or b > 126:
                row[INVALID] += 1
            if cls in (1, 2):
                row[GC] += 1
            if cls == 4:
                row[OTHER] += 1
            row[QUAL_AT + q] += 1
            qsum += q
            if c < CYCLES:
                row[BASE_AT + c * CLASSES + cls] += 1
                row[QSUM_AT + c * CLASSES + cls] += q
        if ls > 0:
            row[READQ_AT + qsum // ls] += 1
    if lengths:
        row[MIN_LEN], row[MAX_LEN] = min(lengths), max(lengths)
    return np.array(row, dtype=np.uint64), 0


# ----------------------------------------------------------- second statement --

_CLASS_LUT = np.full(256, 4, dtype=np.int64)
for _b, _c in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    _CLASS_LUT[_b] = _c
_PHRED_LUT = np.clip(np.arange(256, dtype=np.int64) - 33, 0, 93)
_INVALID_LUT = ((np.arange(256) < 33) | (np.arange(256) > 126)).astype(np.int64)


def row_numpy(text, records):
    """(row uint64[NSTAT], status) of one stream, vectorised."""
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    ends = np.flatnonzero(a == 10).astype(np.int64)
    if len(a) and a[-1] != 10:
        ends = np.append(ends, len(a))
    if len(ends) < 4 * records:
        return zero_row(), VK_EM_BAD_RECORDS
    row = np.zeros(NSTAT, dtype=np.int64)
    if records == 0:
        return row.astype(np.uint64), 0
    ends = ends[:4 * records]
    starts = np.concatenate(([0], ends[:-1] + 1))
    if np.any(a[starts[0::4]] != ord("@")) or np.any(a[starts[2::4]] != ord("+")):
        return zero_row(), VK_QC_BAD_FRAMING
    length = ends - starts
    length -= ((length > 0) & (a[np.maximum(ends - 1, 0)] == 13)).astype(np.int64)
    ls, lq = length[1::4], length[3::4]
    good = ls == lq
    row[RECORDS] = records
    row[RAGGED] = int(np.count_nonzero(~good))
    ls = ls[good]
    s0, q0 = starts[1::4][good], starts[3::4][good]
    if len(ls):
        row[MIN_LEN], row[MAX_LEN] = int(ls.min()), int(ls.max())
        row[LEN_AT:LEN_AT + LEN_BINS] = np.bincount(np.minimum(ls, LEN_BINS - 1), minlength=LEN_BINS)
    total = int(ls.sum())
    row[BASES] = total
    if total:
        read = np.repeat(np.arange(len(ls)), ls)
        cycle = np.arange(total) - np.repeat(np.cumsum(ls) - ls, ls)
        sb, qb = a[s0[read] + cycle], a[q0[read] + cycle]
        cls, q = _CLASS_LUT[sb], _PHRED_LUT[qb]
        row[GC] = int(np.count_nonzero((cls == 1) | (cls == 2)))
        row[OTHER] = int(np.count_nonzero(cls == 4))
        row[INVALID] = int(_INVALID_LUT[qb].sum())
        row[QUAL_AT:QUAL_AT + PHREDS] = np.bincount(q, minlength=PHREDS)
        sums = np.zeros(len(ls), dtype=np.int64)
        np.add.at(sums, read, q)
        has = ls > 0
        row[READQ_AT:READQ_AT + PHREDS] = np.bincount(sums[has] // ls[has], minlength=PHREDS)
        early = cycle < CYCLES
        cell = cycle[early] * CLASSES + cls[early]
        row[BASE_AT:BASE_AT + CYCLES * CLASSES] = np.bincount(cell, minlength=CYCLES * CLASSES)
        qs = np.zeros(CYCLES * CLASSES, dtype=np.int64)
        np.add.at(qs, cell, q[early])
        row[QSUM_AT:QSUM_AT + CYCLES * CLASSES] = qs
    return row.astype(np.uint64), 0


row = row_numpy


def rows(streams):
    """(rows uint64[n, NSTAT], status uint32[n]) of streams [(text, records)]."""
    got = [row_numpy(t, r) for t, r in streams]
    return (np.stack([g[0] for g in got]) if got else np.zeros((0, NSTAT), dtype=np.uint64),
            np.array([g[1] for g in got], dtype=np.uint32))
