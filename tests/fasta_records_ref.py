"""The rule of `--from-fasta --per-record` in plain Python ("--from-fasta --per-record").  Two
statements that share no code: fasta_ref.records gives the joined bytes of every record (and a record's histogram is
fasta_ref.count of a sample that holds it alone); walk() finds starts and names a byte at a time.  They must agree on
how many records a sample has (test_fasta_records_rules.py), and the GPU (vk_fasta_records_count_device,
vk_fasta_records_device, vk_count_fasta_records_device) must equal both exactly."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_ref as FR  # noqa: E402

NAME_BYTES = 128
NO_SLOT = 0xFFFFFFFF


def joined(data):
    """The joined bytes of every record of a sample, in order; none for a sample with a bad start or an empty one."""
    if FR.status(data) or not len(data):
        return []
    return FR.records(data)


def walk(data):
    """[(start, name)] of every record: the offset of its '>' and the bytes of its header line behind it, up to but not
    including the \\n or the sample's end, uncut.  One pass, a byte at a time."""
    data = bytes(data)
    if not data or data[0] != 62:
        return []
    out = []
    line_start, name, in_header = True, None, False
    for i, b in enumerate(data):
        if line_start:
            in_header = b == 62
            if in_header:
                name = bytearray()
                out.append([i, name])
                line_start = False
                continue
        line_start = b == 10
        if in_header and not line_start:
            name.append(b)
    return [(i, bytes(nm)) for i, nm in out]


def kept(name):
    """What the device keeps of a name: NAME_BYTES of it, zero-padded."""
    return name[:NAME_BYTES].ljust(NAME_BYTES, b"\0")


def table(data):
    """[(start, bases, kept name)] of a sample's records."""
    recs, found = joined(data), walk(data)
    assert len(recs) == len(found)
    return [(s, len(r), kept(nm)) for (s, nm), r in zip(found, recs)]


def count(record, k):
    """The histogram (uint32[4^k]) of a record from its joined bytes: that of a sample that holds it alone."""
    return FR.count(b">x\n" + record, k)[0]
