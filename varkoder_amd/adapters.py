"""Adapter sequences of step B (`image --from-raw`): the listed adapters that a detected consensus snaps to, and the
parsing of `--adapter-sequence` / `--adapter-sequence-r2`.  The table is this project's choice (INTEGRATION.md,
"Step B"); the device code keeps the same table in csrc/vk_adapter.h and tests/test_adapter_rules.py checks that the two
agree."""

# (name, sequence) in snapping order: a detected consensus that holds a listed adapter's first 16 bases (or all of it,
# if shorter) becomes that listed sequence, the first match in this order
KNOWN_ADAPTERS = (
    ("Illumina TruSeq read 1", b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"),
    ("Illumina TruSeq read 2", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"),
    ("Nextera / Tn5", b"CTGTCTCTTATACACATCT"),
    ("Illumina small RNA 3'", b"TGGAATTCTCGGGTGCCAAGG"),
)

SNAP_BASES = 16       # bases of a listed adapter that a consensus must hold to snap to it
MIN_LEN, MAX_LEN = 4, 64


def snap(seq):
    """The listed adapter that `seq` holds the head of, or None."""
    for _, ad in KNOWN_ADAPTERS:
        if ad[:SNAP_BASES] in seq:
            return ad
    return None


def parse_adapter(text):
    """An explicit adapter: 4..64 bases of ACGT in any case, stored upper-case.  ValueError otherwise."""
    s = text.encode() if isinstance(text, str) else bytes(text)
    s = s.upper()
    if not (MIN_LEN <= len(s) <= MAX_LEN) or s.strip(b"ACGT"):
        raise ValueError(f"an adapter is {MIN_LEN}..{MAX_LEN} bases of ACGT: {text!r}")
    return s
