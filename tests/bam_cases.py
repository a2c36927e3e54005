"""A BAM writer in plain Python (struct, zlib raw deflate, BGZF members with the `BC` field and the empty EOF member; SAM
spec sections 4.1 and 4.2) and the cases the BAM tests share.  A case is (name, records, header, cut): `records` a list of
record bytes (block_size word included), `header` the header's bytes, `cut` how many bytes are taken off the file's end."""
import functools
import random
import struct
import zlib

CODES = "=ACMGRSVTWYHKDBN"
SMALL_SEG = 256   # VKIMG_BAM_SEG_BYTES of the small-segment engine and emulation


def header(text=b"", refs=()):
    """Magic, l_text, text, n_ref and (name, length) references."""
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return out


def record(name=b"r", seq="", qual=None, flag=4, ref_id=-1, pos=-1, mapq=0, cigar=(), aux=b"", next_ref=-1, next_pos=-1,
           tlen=0, raw_name=None, block_size=None):
    """One record.  seq: letters of CODES; qual: a list of bytes values, None = absent (0xFF per base); cigar: u32 words;
    raw_name: the name field as it is (NUL and all); block_size: a word other than the true one."""
    raw_name = name + b"\0" if raw_name is None else raw_name
    codes = [CODES.index(c) for c in seq]
    packed = bytes((codes[i] << 4) | (codes[i + 1] if i + 1 < len(codes) else 0) for i in range(0, len(codes), 2))
    quals = bytes([0xFF] * len(seq) if qual is None else qual)
    assert len(quals) == len(seq) and len(raw_name) < 256
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(raw_name), mapq, 4680, len(cigar), flag, len(seq), next_ref, next_pos, tlen)
    body += raw_name + b"".join(struct.pack("<I", c) for c in cigar) + packed + quals + aux
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def aux_z(tag, text):
    return tag + b"Z" + text + b"\0"


def aux_bytes(tag, data):
    """A `B` array of bytes that holds `data` as it is."""
    return tag + b"BC" + struct.pack("<I", len(data)) + data


def filler(size, name=b"pad"):
    """A record (no bases: never a read) of exactly `size` bytes, padded with a Z string."""
    n = size - (36 + len(name) + 1) - 4
    assert n >= 0, size
    rec = record(name, aux=aux_z(b"XP", b"p" * n))
    assert len(rec) == size
    return rec


def inflated(records, head, cut=0):
    data = head + b"".join(records)
    return data[:len(data) - cut] if cut else data


def bgzf(data, member=0xFF00):
    """`data` as BGZF: members of at most `member` bytes of text, then the empty EOF member."""
    out = []
    for at in list(range(0, len(data), member)) + [None]:
        chunk = b"" if at is None else data[at:at + member]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out)


def random_read(rng, length, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(length)), [rng.randrange(0, 42) for _ in range(length)]


HD_UNSORTED = b"@HD\tVN:1.6\tSO:unsorted\n"
REFS3 = ((b"chr1", 1000), (b"chr2", 2000), (b"chrM", 16569))


def name_and_length_case():
    """Names of 1 (empty), 2, 3, 4, 5 and 254 bytes with NUL, l_seq 1, 2, 63, 64, 65, 151 and 2000: every alignment 0..3 of
    the fields behind the name, records longer than several small segments, cigars and aux data."""
    rng = random.Random(11)
    recs = []
    for i, name in enumerate((b"", b"a", b"ab", b"abc", b"abcd", b"n" * 253)):
        for j, l in enumerate((1, 2, 63, 64, 65, 151, 2000)):
            seq, qual = random_read(rng, l, "ACGTN" if j % 2 else "ACGT")
            cigar = ((l << 4) | 0,) if (i + j) % 2 else ()
            aux = aux_z(b"RG", b"grp%d" % j) + b"NMC\x03" if (i + j) % 3 == 0 else b""
            mapped = bool(cigar)
            recs.append(record(name, seq, qual, flag=0 if mapped else 4, ref_id=1 if mapped else -1, pos=10 * j if mapped else -1,
                               cigar=cigar, aux=aux))
    return "names_lengths", recs, header(HD_UNSORTED, REFS3), 0


def reverse_case():
    """Reverse reads of odd and even length with every code, absent qualities, a quality above 93."""
    recs = [record(b"rev_odd", "=ACMGRSVTWYHKDBNACG", list(range(20, 39)), flag=0x10, ref_id=0, pos=5, cigar=(19 << 4,)),
            record(b"rev_even", "ACGTTG", [1, 2, 3, 4, 5, 6], flag=0x10, ref_id=2, pos=7, cigar=(6 << 4,)),
            record(b"noqual", "ACGTN", None, flag=4),
            record(b"noqual_rev", "AACGT", None, flag=0x14),
            record(b"hiqual", "ACG", [93, 94, 255], flag=4),
            record(b"noseq", "", [], flag=4)]
    return "reverse", recs, header(HD_UNSORTED, REFS3), 0


def flags_case():
    """Secondary, supplementary, QC-fail and duplicate records among reads of every stream."""
    rng = random.Random(5)
    recs = []
    for i, flag in enumerate((0x4D, 0x8D, 4, 0x100, 0x800, 0x41, 0x81, 0x200 | 4, 0x400 | 4, 0x910, 0xC1, 0x1, 0x40, 0x80, 0x51, 0x91)):
        seq, qual = random_read(rng, 30 + i)
        recs.append(record(b"f%02d" % i, seq, qual, flag=flag))
    return "flags", recs, header(HD_UNSORTED), 0


def seam_cases():
    """A block_size word that starts 0, 1, 2 and 3 bytes before a small segment's seam."""
    rng = random.Random(3)
    head = header(HD_UNSORTED)
    out = []
    for d in range(4):
        seq, qual = random_read(rng, 40)
        recs = [filler(2 * SMALL_SEG - d - len(head))]
        recs += [record(b"s%d_%d" % (d, i), seq, qual) for i in range(12)]
        assert len(head) + len(recs[0]) == 2 * SMALL_SEG - d
        out.append(("seam_%d" % d, recs, head, 0))
    return out


def decoy_case():
    """An aux `B` array that holds eight complete valid records of 42 bytes, placed so that one small segment begins at the
    first of them and the next one inside the seventh: guesses made there pass every test a guess can make, and are
    wrong.  The first of the two segments starts no record; the second does (the host record ends in it), so the link pass
    has to walk it again."""
    rng = random.Random(9)
    head = header(HD_UNSORTED)
    decoys = b"".join(record(b"d%d" % i, *random_read(rng, 2)) for i in range(8))
    assert len(decoys) == 8 * 42
    seq, qual = random_read(rng, 50)
    before = 36 + len(b"host") + 1 + 25 + 50 + 8   # the host record up to its array's bytes: fields, name, bases, qualities, tag
    recs = [filler(3 * SMALL_SEG - before - len(head)), record(b"host", seq, qual, aux=aux_bytes(b"XD", decoys))]
    at = len(head) + len(recs[0]) + before
    assert at == 3 * SMALL_SEG and inflated(recs, head)[at:at + len(decoys)] == decoys
    recs += [record(b"after%d" % i, *random_read(rng, 33)) for i in range(10)]
    return "decoy", recs, head, 0


def empty_cases():
    rng = random.Random(2)
    return [("no_records", [], header(HD_UNSORTED, REFS3), 0),
            ("no_records_no_refs", [], header(), 0),
            ("all_excluded", [record(b"x%d" % i, *random_read(rng, 25), flag=0x100 if i % 2 else 0x800) for i in range(40)],
             header(HD_UNSORTED), 0)]


def first_record_cases():
    """Three files whose first records lie at different offsets (headers of 12, ~60 and ~700 bytes: the last longer than two
    small segments)."""
    rng = random.Random(4)
    heads = (header(), header(HD_UNSORTED, REFS3), header(HD_UNSORTED + b"@CO\t" + b"c" * 600 + b"\n", REFS3))
    return [("first_%d" % i, [record(b"q%d_%d" % (i, j), *random_read(rng, 20 + 7 * j)) for j in range(20)], h, 0)
            for i, h in enumerate(heads)]


def error_cases():
    """A last record cut short; a block_size too small for its fields; an empty name; a name without NUL."""
    rng = random.Random(6)
    good = [record(b"g%d" % i, *random_read(rng, 45)) for i in range(15)]
    head = header(HD_UNSORTED)
    seq, qual = random_read(rng, 30)
    small = record(b"small", seq, qual)
    small = struct.pack("<i", 32 + 6 + 15 + 29) + small[4:]   # (one byte short of its qualities)
    return [("truncated", good, head, 7),
            ("truncated_in_word", good, head, len(good[-1]) - 2),
            ("bad_block_size", good[:9] + [small] + good[9:], head, 0),
            ("block_size_under_32", good[:3] + [struct.pack("<i", 8) + b"\0" * 8] + good[3:], head, 0),
            ("empty_name_field", good[:5] + [record(raw_name=b"", seq=seq, qual=qual)], head, 0),
            ("name_without_nul", good[:5] + [record(raw_name=b"abc", seq=seq, qual=qual)] + good[5:], head, 0)]


def bulk_case():
    """1,500 reads of 50 to 250 bases, about 300 KB: several segments at the default size, more than a thousand small
    ones; single reads, mates, reverse reads and excluded records mixed."""
    rng = random.Random(8)
    recs = []
    for i in range(1500):
        seq, qual = random_read(rng, rng.randrange(50, 251))
        flag = (4, 0x4D, 0x8D, 0x10, 0x100, 0x51)[rng.randrange(6)]
        recs.append(record(b"bulk.%d" % i, seq, qual, flag=flag, aux=aux_z(b"RG", b"g") if i % 5 == 0 else b""))
    return "bulk", recs, header(HD_UNSORTED, REFS3), 0


@functools.lru_cache(maxsize=None)
def unit_cases():
    """Every case the emulation and the GPU tests convert: [(name, inflated bytes)]."""
    cases = [name_and_length_case(), reverse_case(), flags_case()] + seam_cases() + [decoy_case()] + empty_cases() + \
        first_record_cases() + error_cases() + [bulk_case()]
    return [(name, inflated(recs, head, cut)) for name, recs, head, cut in cases]


def synthetic_reads(seed, n, length=100):
    """n reads [(name, seq, qual)] of a random 3 kb genome's fragments: enough shared sequence for step B to have work."""
    rng = random.Random(seed)
    genome = "".join(rng.choice("ACGT") for _ in range(3000))
    out = []
    for i in range(n):
        at = rng.randrange(0, len(genome) - length)
        out.append((b"read%d_%d" % (seed, i), genome[at:at + length], [rng.randrange(25, 41) for _ in range(length)]))
    return out


def fastq_text(reads):
    return b"".join(b"@" + n + b"\n" + s.encode() + b"\n+\n" + bytes(q + 33 for q in qual) + b"\n" for n, s, qual in reads)


def revcomp(seq):
    return seq[::-1].translate(str.maketrans("ACGT", "TGCA"))
