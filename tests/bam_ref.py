"""The rule of `--from-bam` ("--from-bam: the rule") in plain Python, written from the rule and the SAM
spec (section 4.2), not from the product's code: inflated BAM bytes -> the FASTQ text of every stream and the file's
status.  One record at a time, in order; no segments, no guesses."""
import struct

BAD_RECORD, TRUNCATED = 1, 2
ALL, READ1, READ2, SINGLE = 0, 1, 2, 3
EXCLUDE_DEFAULT = 0x900

LETTERS = "NACMGRSVTWYHKDBN"   # "=ACMGRSVTWYHKDBN" with '=' written as N
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C", "M": "K", "K": "M", "R": "Y", "Y": "R", "V": "B", "B": "V", "H": "D",
              "D": "H", "S": "S", "W": "W", "N": "N"}


def header_end(data):
    """The offset of the first record: behind magic, l_text, text, n_ref and the references.  Returns (offset, n_ref)."""
    assert data[:4] == b"BAM\x01"
    (l_text,) = struct.unpack_from("<i", data, 4)
    at = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, at)
    at += 4
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, at)
        at += 4 + l_name + 4
    return at, n_ref


def read_text(name, codes, quals, flag):
    """One read's FASTQ text from its name (without NUL), 4-bit base codes, quality bytes and flag."""
    seq = "".join(LETTERS[c] for c in codes)
    if quals and quals[0] == 0xFF:
        qual = "I" * len(codes)
    else:
        qual = "".join(chr(min(q, 93) + 33) for q in quals)
    if flag & 0x10:
        seq = "".join(COMPLEMENT[b] for b in reversed(seq))
        qual = qual[::-1]
    return b"@" + name + b"\n" + seq.encode() + b"\n+\n" + qual.encode("latin-1") + b"\n"


def stream_of(flag):
    return READ1 if flag & 0xC1 == 0x41 else READ2 if flag & 0xC1 == 0x81 else SINGLE


def convert(data, first_record, exclude=EXCLUDE_DEFAULT):
    """(status, {ALL: text, READ1: text, READ2: text, SINGLE: text}, {select: reads}) of one file's inflated bytes.  With
    a status every text is empty."""
    data = bytes(data)
    n = len(data)
    texts = {s: [] for s in (ALL, READ1, READ2, SINGLE)}
    status = 0
    at = first_record
    if at > n:
        status = TRUNCATED
    while not status and at < n:
        if at + 4 > n:
            status = TRUNCATED
            break
        (block_size,) = struct.unpack_from("<i", data, at)
        if block_size < 32:
            status = BAD_RECORD
            break
        if at + 4 + block_size > n:
            status = TRUNCATED
            break
        b = data[at + 4:at + 4 + block_size]
        _ref, _pos, l_name, _mapq, _bin, n_cigar, flag, l_seq, _nref, _npos, _tlen = struct.unpack_from("<iiBBHHHIiii", b, 0)
        need = 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
        if block_size < need or l_name == 0 or b[32 + l_name - 1] != 0:
            status = BAD_RECORD
            break
        if l_seq > 0 and flag & exclude == 0:
            name = b[32:32 + l_name - 1]
            s0 = 32 + l_name + 4 * n_cigar
            packed = b[s0:s0 + (l_seq + 1) // 2]
            codes = [(packed[i >> 1] >> 4) if i % 2 == 0 else (packed[i >> 1] & 15) for i in range(l_seq)]
            quals = b[s0 + (l_seq + 1) // 2:s0 + (l_seq + 1) // 2 + l_seq]
            text = read_text(name, codes, quals, flag)
            assert len(text) == l_name + 2 * l_seq + 5
            texts[ALL].append(text)
            texts[stream_of(flag)].append(text)
        at += 4 + block_size
    if status:
        texts = {s: [] for s in texts}
    return status, {s: b"".join(t) for s, t in texts.items()}, {s: len(t) for s, t in texts.items()}
