"""The cases the read-group tests share, built with tests/bam_cases.py (record, aux_z, aux_bytes): [(name, inflated bytes,
the file's group IDs)].  Each is a few KiB (the 1024-group one about 70: its header alone is 50), so that segments of 256
bytes and of 65536 both see seams, and panels of a few small segments do too."""
import functools
import random
import struct

import bam_cases as BC

SMALL_PANEL = 3   # VKIMG_BAM_PANEL_SEGS of the small-segment engine and emulation


def rg_header(ids, refs=()):
    text = BC.HD_UNSORTED + b"".join(b"@RG\tID:" + i + b"\tSM:specimen\tPL:ONT\n" for i in ids)
    return BC.header(text, refs)


def rg(value):
    return BC.aux_z(b"RG", value)


def read(rng, name, aux=b"", flag=4, length=None):
    seq, qual = BC.random_read(rng, length or rng.randrange(8, 40))
    return BC.record(name, seq, qual, flag=flag, aux=aux)


def ids_of(n):
    return [b"run7_sup@v5_barcode%02d" % i for i in range(n)]


def count_cases():
    """1, 2, 3, 65 and 1024 groups: reads that cycle through the groups (the 1024: every fifth, the first and the last
    among them), one read in seven without RG."""
    out = []
    for n in (1, 2, 3, 65, 1024):
        rng = random.Random(100 + n)
        ids = ids_of(n)
        picks = list(range(n)) if n < 1024 else [0, 1023] + list(range(3, 1024, 5))
        recs = []
        for i in range(max(150, len(picks))):
            aux = b"" if i % 7 == 3 else rg(ids[picks[i % len(picks)]]) + b"NMC\x02"
            recs.append(read(rng, b"c%d.%d" % (n, i), aux))
        out.append(("groups_%d" % n, BC.inflated(recs, rg_header(ids)), ids))
    return out


def placement_case():
    """A group whose only read is the file's first record, one whose only read is its last, one without reads; 70
    consecutive reads of one group; two groups that alternate at every record for 150 records."""
    rng = random.Random(21)
    ids = [b"first", b"last", b"none", b"run", b"even", b"odd"]
    recs = [read(rng, b"only_first", rg(b"first"))]
    recs += [read(rng, b"run%d" % i, rg(b"run")) for i in range(70)]
    recs += [read(rng, b"alt%d" % i, rg(b"odd" if i % 2 else b"even")) for i in range(150)]
    recs += [read(rng, b"only_last", rg(b"last"))]
    return "placement", BC.inflated(recs, rg_header(ids)), ids


def nomatch_case():
    """Reads without RG; values that are no ID: not in the table, a proper prefix of an ID, an ID a proper prefix of the
    value, IDs that differ in the last byte only, the empty value, a value of 300 bytes; RG of type A and of type i (the
    first RG decides: a good RG:Z behind it does not count)."""
    rng = random.Random(22)
    ids = [b"lib_a", b"lib_b", b"library", b"x"]
    values = [None, b"other", b"lib_", b"lib", b"lib_ab", b"lib_c", b"", b"libr", b"library1", b"xx", b"lib_a" + b"a" * 295,
              b"lib_a", b"lib_b", b"library", b"x"]
    recs = []
    for i in range(90):
        v = values[i % len(values)]
        recs.append(read(rng, b"v%d" % i, b"" if v is None else b"XSi" + struct.pack("<i", i) + rg(v)))
    recs.append(read(rng, b"typeA", b"RGAx" + rg(b"x")))
    recs.append(read(rng, b"typei", b"RGi" + struct.pack("<i", 7) + rg(b"lib_a")))
    recs.append(read(rng, b"after", rg(b"lib_b")))
    return "nomatch", BC.inflated(recs, rg_header(ids)), ids


def behind_case():
    """RG behind one field of every type and every B subtype, a B of count 0, a B of 700 bytes (longer than two small
    segments); a Z value that holds `RGZ<an ID>\\0` in front of the true RG field."""
    rng = random.Random(23)
    ids = [b"g0", b"g1", b"g2"]
    fields = [b"XAA!", b"Xcc\x80", b"XCC\xff", b"Xss" + struct.pack("<h", -2), b"XSS" + struct.pack("<H", 65535),
              b"Xii" + struct.pack("<i", -5), b"XII" + struct.pack("<I", 4000000000), b"Xff" + struct.pack("<f", 1.5),
              BC.aux_z(b"XZ", b"some text"), BC.aux_z(b"XZ", b""), b"XHH1AE301\0"]
    for sub, size in ((b"c", 1), (b"C", 1), (b"s", 2), (b"S", 2), (b"i", 4), (b"I", 4), (b"f", 4)):
        fields.append(b"XBB" + sub + struct.pack("<I", 3) + bytes(range(3 * size)))
        fields.append(b"X0B" + sub + struct.pack("<I", 0))
    fields.append(BC.aux_bytes(b"XL", bytes(rng.randrange(256) for _ in range(700))))
    fields.append(BC.aux_z(b"XT", b"RGZg0") + b"")            # the bytes R G Z g 0 NUL inside a value
    fields.append(BC.aux_bytes(b"XD", b"RGZg1\0RGZg1\0"))     # and inside an array
    recs = []
    for i, f in enumerate(fields):
        recs.append(read(rng, b"b%d" % i, f + rg(ids[(i + 2) % 3])))
        recs.append(read(rng, b"n%d" % i, f))                 # the same field and no RG: ungrouped
    recs.append(read(rng, b"all", b"".join(fields) + rg(b"g2")))
    return "behind", BC.inflated(recs, rg_header(ids)), ids


def bad_aux_cases():
    """Each way an aux area can be bad in front of the deciding field: status 3."""
    ids = [b"g0", b"g1"]
    bad = {"bad_type": b"XXq\x01" + rg(b"g0"),
           "bad_subtype": b"XBBZ" + struct.pack("<I", 1) + b"\0" + rg(b"g0"),
           "bad_subtype_A": b"XBBA" + struct.pack("<I", 1) + b"A" + rg(b"g0"),
           "z_without_nul": b"XZZno end",
           "h_without_nul": b"XHH1A",
           "b_count_past_block": b"XBBi" + struct.pack("<I", 1000) + b"\0" * 40,
           "b_count_huge": b"XBBI" + struct.pack("<I", 0xFFFFFFFF) + b"\0" * 8,
           "b_header_cut": b"XBBc\x01\0",
           "fixed_past_block": b"Xii\x01\x02",
           "stray_1": b"XCC\x01" + b"R",
           "stray_2": b"XCC\x01" + b"RG"}
    out = []
    for k, (name, aux) in enumerate(sorted(bad.items())):
        rng = random.Random(300 + k)
        recs = [read(rng, b"ok%d" % i, rg(ids[i % 2])) for i in range(25)]
        recs.insert(17, read(rng, b"bad", aux))
        out.append((name, BC.inflated(recs, rg_header(ids)), ids))
    return out


def ignored_bad_case():
    """Bad aux that must be ignored: behind the deciding field, in a record that `exclude` drops, in a record without
    bases."""
    rng = random.Random(24)
    ids = [b"g0", b"g1"]
    recs = []
    for i in range(40):
        recs.append(read(rng, b"ok%d" % i, rg(ids[i % 2])))
        if i % 8 == 1:
            recs.append(read(rng, b"tail%d" % i, rg(ids[i % 2]) + b"XXq\x01\x02"))
        if i % 8 == 3:
            recs.append(read(rng, b"tailA%d" % i, b"RGAx" + b"X"))           # (type A decides: the stray byte is behind it)
        if i % 8 == 5:
            recs.append(read(rng, b"sec%d" % i, b"XZZno end", flag=0x100))
        if i % 8 == 7:
            recs.append(BC.record(b"nobases%d" % i, aux=b"XBBi" + struct.pack("<I", 99)))
    return "ignored_bad", BC.inflated(recs, rg_header(ids)), ids


def pairs_case():
    """Mates of pairs spread over groups, single reads and excluded records in between."""
    rng = random.Random(25)
    ids = [b"bc01", b"bc02", b"bc03"]
    recs = []
    for i in range(60):
        g = ids[i % 3]
        recs.append(read(rng, b"p%d" % i, rg(g), flag=0x4D))
        recs.append(read(rng, b"p%d" % i, rg(ids[(i + i // 3) % 3]) if i % 5 else b"", flag=0x8D))
        if i % 4 == 0:
            recs.append(read(rng, b"s%d" % i, rg(g), flag=4 if i % 8 else 0x14))
        if i % 6 == 0:
            recs.append(read(rng, b"x%d" % i, rg(g), flag=0x900))
    return "pairs", BC.inflated(recs, rg_header(ids, BC.REFS3)), ids


def status_cases():
    """A file cut short and a bad record, each with bad aux in front of it: the framing's status comes first.  A file
    without @RG lines; a file without records."""
    rng = random.Random(26)
    ids = [b"g0", b"g1"]
    good = [read(rng, b"ok%d" % i, rg(ids[i % 2])) for i in range(30)]
    bad = read(rng, b"bad", b"XXq\x01")
    head = rg_header(ids)
    return [("truncated", BC.inflated(good, head, 9), ids),
            ("truncated_bad_aux", BC.inflated(good[:10] + [bad] + good[10:], head, 9), ids),
            ("bad_record_bad_aux", BC.inflated(good[:5] + [bad] + good[5:20] + [struct.pack("<i", 8) + b"\0" * 8], head), ids),
            ("no_groups", BC.inflated(good, BC.header(BC.HD_UNSORTED)), []),
            ("no_records", BC.inflated([], head), ids)]


@functools.lru_cache(maxsize=None)
def unit_cases():
    """Every case the emulation and the GPU tests convert: [(name, inflated bytes, ids)]."""
    return count_cases() + [placement_case(), nomatch_case(), behind_case()] + bad_aux_cases() + \
        [ignored_bad_case(), pairs_case()] + status_cases()

