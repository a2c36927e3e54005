"""The rule of `--exclude-fasta` / `--keep-fasta` in plain Python ("--exclude-fasta / --keep-fasta: the
rule"), stated twice.  vk_screen_build_device and vk_screen_device must equal it exactly.

The set.  K is 16..31.  The reference is one FASTA text; its lines, headers and records are read by the rules of
`--from-fasta` (tests/fasta_ref.py): a line ends at \\n, a \\r directly before it (or as the text's last byte) belongs to
the line end, a line that begins with '>' is a header, the other lines join into the current record.  A base is ACGT of
either case, coded 0 1 2 3.  Any other sequence byte, and every record boundary, breaks the sequence; no k-mer spans a
break.  Every window of K unbroken bases gives a key: the smaller of the window and its reverse complement, read as 2K-bit
integers, first base most significant.  The set is the distinct keys; it may be empty.

A read.  Its windows are taken the same way from its sequence line, as the bytes stand in the FASTQ text (a \\r that ends
the line is no part of it).  Its hits are the number of window POSITIONS whose key is in the set.  It matches when hits >=
min_hits (>= 1).  A read of fewer than K bases never matches.

A sample.  Record by record: four lines.  exclude keeps the records that do not match, keep those that do; a kept record
is copied byte for byte (a \\r included, a last line without \\n as it is), in input order.  stats = records in, records
kept, sequence bases in, sequence bases kept (the sequence line's bytes without its \\r, every class).  Framing is the
read index's (VK_ST_*, as vk_ladder_emit_device reports them): a sample with a status gets no text and zero stats.

First statement (strings): set_strings / hits_strings -- the upper-cased windows of the reference's records and their
reverse complements as a Python set of strings; a read's window hits when the string is in it.
Second statement (integers): set_ints / hits_ints -- one walk over the bytes with rolling 2-bit keys, forward and reverse
complement, no line splitting; shares no code with the first.  tests/test_screen_rules.py holds the two to each other."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_ref  # noqa: E402

VK_ST_BAD_START, VK_ST_BAD_PHASE, VK_EM_BAD_RECORDS = 1, 2, 8
K_MIN, K_MAX = 16, 31
MIN_SLOTS = 1024

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def revcomp(w):
    return w.translate(_COMP)[::-1]


def key_of(w):
    """The key of a window given as a string of ACGT: the smaller of it and its reverse complement, as an integer."""
    return min(int(w.translate(bytes.maketrans(b"ACGT", b"0123")), 4), int(revcomp(w).translate(bytes.maketrans(b"ACGT", b"0123")), 4))


# ------------------------------------------------------------ first statement --

def _windows(seq, k):
    """(position, upper-case window) of every window of k bytes of seq that holds bases only."""
    up = bytes(seq).upper()
    for i in range(len(up) - k + 1):
        w = up[i:i + k]
        if not w.strip(b"ACGT"):
            yield i, w


def set_strings(fasta, k):
    """The windows of the reference's records and their reverse complements."""
    out = set()
    for rec in fasta_ref.records(fasta):
        for _, w in _windows(rec, k):
            out.add(w)
            out.add(revcomp(w))
    return out


def distinct_strings(strings):
    return len({min(w, revcomp(w)) for w in strings})


def hits_strings(seq, strings, k):
    return sum(1 for _, w in _windows(seq, k) if w in strings)


# ----------------------------------------------------------- second statement --

def _roll(codes, k):
    """The key of every window of k codes that ends at position i of `codes` (None: a break): (i, key)."""
    mask = (1 << (2 * k)) - 1
    fw = rc = run = 0
    for i, c in enumerate(codes):
        if c is None:
            run = 0
            continue
        fw = ((fw << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * k - 2))
        run += 1
        if run >= k:
            yield i, min(fw, rc)


def _fasta_codes(data):
    """The reference's sequence bytes as codes, a None for every non-base and at every header line: one walk over the
    bytes with the state a reader of the rule would keep."""
    data = bytes(data)
    n = len(data)
    out = []
    line_start, header = True, False
    for i, b in enumerate(data):
        if line_start:
            header = b == 62
            line_start = False
            if header:
                out.append(None)
        if b == 10:
            line_start = True
            continue
        if header:
            continue
        if b == 13 and (i + 1 == n or data[i + 1] == 10):
            continue
        out.append(_CODE.get(b))
    return out


def set_ints(fasta, k):
    """The distinct keys of the reference as a set of integers."""
    return {key for _, key in _roll(_fasta_codes(fasta), k)}


def windows_ints(fasta, k):
    """The number of windows of k unbroken bases of the reference (what sizes the table)."""
    return sum(1 for _ in _roll(_fasta_codes(fasta), k))


def hits_ints(seq, keys, k):
    return sum(1 for _, key in _roll([_CODE.get(b) for b in bytes(seq)], k) if key in keys)


def slots_for(windows):
    """The table's size: a power of two, at least twice the number of windows and at least 1,024."""
    n = MIN_SLOTS
    while n < 2 * windows:
        n *= 2
    return n


def ref_status(fasta):
    return fasta_ref.status(fasta)


# -------------------------------------------------------------------- samples --

def split_records(text):
    """(status, [(the record's bytes, its sequence line without a trailing \\r)]) of a cleaned FASTQ text."""
    text = bytes(text)
    if not text:
        return 0, []
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    status = 0
    if text[:1] != b"@":
        status |= VK_ST_BAD_START
    if len(lines) % 4:
        status |= VK_ST_BAD_PHASE
    if len(lines) >= 3 and lines[2][:1] != b"+":
        status |= VK_ST_BAD_START
    if status:
        return status, []
    out, at = [], 0
    for r in range(len(lines) // 4):
        n = sum(len(ln) + 1 for ln in lines[4 * r:4 * r + 4])
        raw = text[at:at + n]      # (the last record may lack its \n: the slice ends with the text)
        at += n
        seq = lines[4 * r + 1]
        out.append((raw, seq[:-1] if seq.endswith(b"\r") else seq))
    return 0, out


def screen(text, the_set, k, min_hits=1, keep=False, hits=None):
    """(kept text, [records in, records kept, bases in, bases kept], status) of a sample.  the_set: set_strings' or
    set_ints' result; hits: hits_strings or hits_ints (None: by the set's element type)."""
    if hits is None:
        hits = hits_strings if any(isinstance(x, bytes) for x in the_set) else hits_ints
    status, recs = split_records(text)
    if status:
        return b"", [0, 0, 0, 0], status
    out = bytearray()
    stats = [0, 0, 0, 0]
    for raw, seq in recs:
        match = hits(seq, the_set, k) >= min_hits
        stats[0] += 1
        stats[2] += len(seq)
        if match == bool(keep):
            out += raw
            stats[1] += 1
            stats[3] += len(seq)
    return bytes(out), stats, 0
