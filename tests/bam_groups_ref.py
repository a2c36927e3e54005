"""The rule of `--from-bam --bam-read-groups` ("--from-bam --bam-read-groups: the rule") in plain Python on
top of tests/bam_ref.py, written from the rule and the SAM spec (sections 1.3 and 4.2.4), not from the product's code:
inflated BAM bytes and the file's group IDs -> the FASTQ text of every (select, group) and the file's status.  One record
at a time, in order."""
import struct

import bam_ref as BR

BAD_AUX = 3
UNGROUPED = 0xFFFFFFFF
MAX_GROUPS = 1024
FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
ELEM = {k: v for k, v in FIXED.items() if k != b"A"}


class BadAux(Exception):
    pass


def header_groups(text):
    """The IDs of the @RG lines of a header's text, in order (no checks: the product's bam.read_groups has them)."""
    ids = []
    for line in text.split(b"\n"):
        if line.startswith(b"@RG\t") or line == b"@RG":
            for field in line.rstrip(b"\r").split(b"\t")[1:]:
                if field.startswith(b"ID:"):
                    ids.append(field[3:])
                    break
    return ids


def group_of(aux, ids):
    """The group of a read whose aux area is `aux`: an index into ids or UNGROUPED; BadAux for a field in front of the
    deciding one that does not parse."""
    at, n = 0, len(aux)
    while at < n:
        if n - at < 3:
            raise BadAux("stray bytes")
        tag, kind = aux[at:at + 2], aux[at + 2:at + 3]
        at += 3
        if tag == b"RG":
            if kind != b"Z":
                return UNGROUPED
            end = aux.find(b"\0", at)
            if end < 0:
                return UNGROUPED
            value = aux[at:end]
            return ids.index(value) if value in ids else UNGROUPED
        if kind in FIXED:
            if n - at < FIXED[kind]:
                raise BadAux("a value past the block")
            at += FIXED[kind]
        elif kind in (b"Z", b"H"):
            end = aux.find(b"\0", at)
            if end < 0:
                raise BadAux("no NUL")
            at = end + 1
        elif kind == b"B":
            if n - at < 5:
                raise BadAux("a B header past the block")
            sub = aux[at:at + 1]
            (count,) = struct.unpack_from("<I", aux, at + 1)
            at += 5
            if sub not in ELEM:
                raise BadAux("unknown subtype")
            if n - at < count * ELEM[sub]:
                raise BadAux("a B array past the block")
            at += count * ELEM[sub]
        else:
            raise BadAux("unknown type")
    return UNGROUPED


def convert(data, first_record, ids, exclude=BR.EXCLUDE_DEFAULT, notes=None):
    """(status, {(select, group): text}) of one file's inflated bytes: a key for every select of ALL, READ1, READ2, SINGLE
    and every group of range(len(ids)) and UNGROUPED that has reads; with a status the dict is empty.  notes (a list):
    gets (class or 0, group or None) per record."""
    status, _, _ = BR.convert(data, first_record, exclude)
    if status:
        return status, {}
    data = bytes(data)
    texts = {}
    at = first_record
    while at < len(data):
        (block_size,) = struct.unpack_from("<i", data, at)
        b = data[at + 4:at + 4 + block_size]
        _ref, _pos, l_name, _mapq, _bin, n_cigar, flag, l_seq, _nref, _npos, _tlen = struct.unpack_from("<iiBBHHHIiii", b, 0)
        if l_seq > 0 and flag & exclude == 0:
            s0 = 32 + l_name + 4 * n_cigar
            packed = b[s0:s0 + (l_seq + 1) // 2]
            codes = [(packed[i >> 1] >> 4) if i % 2 == 0 else (packed[i >> 1] & 15) for i in range(l_seq)]
            q0 = s0 + (l_seq + 1) // 2
            text = BR.read_text(b[32:32 + l_name - 1], codes, b[q0:q0 + l_seq], flag)
            try:
                group = group_of(b[q0 + l_seq:], ids)
            except BadAux:
                return BAD_AUX, {}
            cls = BR.stream_of(flag)
            for select in (BR.ALL, cls):
                texts.setdefault((select, group), []).append(text)
            if notes is not None:
                notes.append((cls, group))
        elif notes is not None:
            notes.append((0, None))
        at += 4 + block_size
    return 0, {k: b"".join(v) for k, v in texts.items()}
