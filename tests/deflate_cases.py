"""The texts that the BGZF compressor's tests share (tests/test_gpu_deflate.py on the GPU, tests/test_deflate_emulation.py
on the host emulation) and what every compressed file must satisfy.  zlib is the judge, never the code under test."""
import hashlib
import os
import struct
import zlib

import numpy as np

import fastq_cases

MEMBER = 65280            # text bytes of a member at most
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
TABLE_ALLOWANCE = 286     # 14 + 19*3 + 316*7 bits: what sending the code lengths without run-length symbols may cost
FRAMING = 26              # 18 bytes of header, CRC-32 and ISIZE


def fib(i):
    a, b = 1, 1
    for _ in range(i):
        a, b = b, a + b
    return a


def record300():
    """One FASTQ record of exactly 300 bytes."""
    rng = np.random.default_rng(300)
    head = b"@M00001:7:000000000-ABCDE:1:1101:15589:1332 1:N:0:1"
    n = (300 - len(head) - 5) // 2
    seq = bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    qual = bytes(rng.choice(list(b"FFFFF:,#"), size=n).astype(np.uint8))
    r = head + b"\n" + seq + b"\n+\n" + qual + b"\n"
    r = r[:1] + b"x" * (300 - len(r)) + r[1:]
    assert len(r) == 300
    return r


def texts():
    """name -> text.  Names that start with fastq_, and `skewed` and `repeated`, also get the size checks."""
    rng = np.random.default_rng(20240)
    t = {}
    t["empty"] = b""
    t["one_byte"] = b"A"
    for n in (MEMBER - 1, MEMBER, MEMBER + 1, 2 * MEMBER + 1):
        # FASTQ-like filler: compressible, not periodic
        t[f"boundary_{n}"] = bytes(rng.choice(list(b"ACGT\nI@+"), size=n, p=[.2, .2, .2, .2, .02, .14, .02, .02]).astype(np.uint8))
    t["random"] = rng.integers(0, 256, MEMBER, dtype=np.uint8).tobytes()
    t["one_value"] = b"G" * MEMBER
    t["repeated"] = record300() * 200
    # 1,000 random bytes again at distance exactly 32,768 (the farthest DEFLATE can state: distance symbol 29 with all 13
    # extra bits), and 1,000 others again at 32,769 (one too far).  One repeated byte fills the rest, so the first
    # block's positions stay in the matcher's table until its copy comes.
    far = bytearray(b"." * 34769)
    far[0:2000] = rng.integers(0, 256, 2000, dtype=np.uint8).tobytes()
    far[32768:33768] = far[0:1000]
    far[33769:34769] = far[1000:2000]
    t["far"] = bytes(far)
    t["uniform256"] = bytes(range(256)) * 64
    skew = np.concatenate([np.full(fib(i), i, dtype=np.uint8) for i in range(22)])
    assert len(skew) == 46367
    np.random.default_rng(22).shuffle(skew)
    t["skewed"] = skew.tobytes()
    for name, body in fastq_cases.edge_cases().items():
        if body:
            t["fastq_" + name] = body
    return t


def small_files():
    """300 small files, every seventh of zero bytes."""
    rng = np.random.default_rng(300300)
    out = []
    for i in range(300):
        n = 0 if i % 7 == 3 else int(rng.integers(1, 400))
        out.append(bytes(rng.choice(list(b"ACGTN\n@+I#"), size=n).astype(np.uint8)))
    return out


def fastq_like(rng, n):
    """n bytes of FASTQ records (reads of 40..250 bases, Illumina-like headers, qualities over a few values)."""
    out, size, i = [], 0, 0
    while size < n:
        m = int(rng.integers(40, 251))
        seq = bytes(rng.choice(list(b"ACGTN"), size=m, p=[.245, .245, .245, .245, .02]).astype(np.uint8))
        qual = bytes(rng.choice(list(b"FFFF:,#"), size=m).astype(np.uint8))
        r = b"@M0%d:7:000-ABCDE:1:%d:%d:%d 1:N:0:1\n" % (int(rng.integers(1, 5)), 1101 + i % 7, int(rng.integers(1000, 30000)),
                                                         int(rng.integers(1000, 30000)))
        r += seq + b"\n+\n" + qual + b"\n"
        out.append(r)
        size += len(r)
        i += 1
    return b"".join(out)[:n]


PERIODS = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 258, 259, 300, 511, 512, 513, 4095, 4096, 4097)
# both sides of every distance symbol's first distance: 1..9, 12, 13, then 2^k and 3 * 2^(k-1) and the distance behind each
DISTANCES = sorted(set(list(range(1, 10)) + [12, 13] +
                       [d + e for k in range(4, 16) for d in (2 ** k, 3 * 2 ** (k - 1)) for e in (0, 1) if d + e <= 32768]))
FUZZ = 300


def _random(rng, n, avoid=()):
    """n random bytes, none of them in `avoid`"""
    ok = np.array([v for v in range(256) if v not in avoid], dtype=np.uint8)
    return ok[rng.integers(0, len(ok), size=n)].tobytes()


def _distance_text(rng, d):
    """A 40-byte chunk again at distance exactly d (d < 40: a unit of d different bytes over 200 bytes), in bytes drawn
    from 48 values, so that a block with codes is smaller than the stored one and the matches are written.  The
    matcher sees an occurrence only from the round (256 positions) after it, and only while no later position took its
    place in the hash table: the second chunk starts a round, and a long way between the two is one repeated byte
    (which the chunk and its neighbours do not hold), as in texts()["far"]."""
    def some(n):
        return (rng.integers(0, 48, size=n, dtype=np.uint8) + 64).tobytes()
    if d < 40:
        unit = (rng.permutation(48)[:d].astype(np.uint8) + 64).tobytes()
        return some(600) + (unit * (200 // d + 1))[:200] + some(50)
    second = -(-(600 + d) // 256) * 256
    chunk = some(40)
    between = some(d - 40) if d <= 2049 else b"." * (d - 40)
    return some(second - d) + chunk + between + chunk + some(50)


def _skewed_with_matches():
    """A stream of matches and almost nothing else whose literal/length code is deeper than 15 bits without the limit:
    runs of A, B, C, A ... of 9, 10, 11 ... 31 bytes.  From the hash table the matcher knows the last four bytes of the
    letter's last run in an earlier round, so a run becomes a match of 4 from there and a match of its other 5, 6, 7
    ... 27 bytes at distance 1: one length symbol per run length, and the lengths' counts grow so that each is a little
    more than all the rarer ones together (8, 8, 16, 25, 42 ... 2237; the longest run is the rarest).  No run lies
    across a round's border (the letter's next runs would meet its middle there): every round is filled to its 256
    bytes with runs of 9 and 10.  Round 0 is three long runs, so that the literals are one A, one B and one C."""
    rng = np.random.default_rng(1952)
    counts = [8, 8]
    while len(counts) < 13:   # bottom of the tree (A, B, C, end of block, round 0's length): 7
        below = 7 + sum(counts[:-1])
        counts.append(below + max(2, below // 16))
    runs = [27, 23, 19, 17, 15, 13, 11, 10, 9, 8, 7, 6, 5]   # match lengths 259 ... 271's; a run is 4 more
    others = np.concatenate([np.full(c, L + 4) for c, L in zip(counts[:-2], runs[:-2])])
    rng.shuffle(others)
    others = others.tolist()
    n10, n9 = counts[-2], counts[-1]
    rounds = []
    while others or n9 or n10:
        this, room = [], 256
        while others and room - others[-1] >= 120:
            this.append(others.pop())
            room -= this[-1]
        # room = 9 a + 10 b: b = room mod 9 (+ 9, + 18 ...), whichever keeps the two supplies in proportion
        want = room * n10 / max(1, 9 * n9 + 10 * n10)
        fits = [b for b in range(room % 9, room // 10 + 1, 9) if b <= n10 and (room - 10 * b) // 9 <= n9]
        if not fits:   # the supplies end: what is left goes into the last round as it is
            this += [10] * n10 + [9] * n9 + others
            n9 = n10 = 0
            others = []
        else:
            b = min(fits, key=lambda b: abs(b - want))
            a = (room - 10 * b) // 9
            fill = [10] * b + [9] * a
            n10, n9 = n10 - b, n9 - a
            this += fill
            order = rng.permutation(len(this))
            this = [this[i] for i in order]
        rounds.append(this)
    out = bytearray(b"A" * 85 + b"B" * 85 + b"C" * 86)
    j = 0
    for r in rounds:
        for n in r:
            out += b"ABC"[j % 3:j % 3 + 1] * n
            j += 1
    assert len(out) <= MEMBER, len(out)
    return bytes(out)


def _skewed_distances():
    """Distance symbols used in Fibonacci proportions (1, 1, 2, 3, 5 ... over 17 symbols, each count a little over the
    sum of the two before), so that the distance code needs the 15-bit limit.  How a match at distance exactly d is
    made, given that the matcher sees only earlier rounds (and distance 1): d >= 256 as blocks of d bytes, each the
    block before with one byte in five changed (matches of 4 at distance d); d < 256 as the first bytes of a round,
    copied the same way from the end of the round before; distance 1 as runs of four equal bytes, every run of another
    value (a second run of a value would match the first through the hash table instead)."""
    rng = np.random.default_rng(1951)
    order = [6, 8, 12, 16, 24, 32, 48, 64, 96, 1, 128, 192, 256, 896, 640, 448, 320]
    counts = [1, 1]   # a little more than the two before together: a match that is not found does not end the chain
    while len(counts) < len(order):
        counts.append(counts[-1] + counts[-2] + counts[-1] // 16)
    out = bytearray()

    def copy(d, k, g=4):   # k groups of 5 bytes from distance d, byte g of each changed: matches of 4 between the changes
        for i in range(5 * k):
            out.append(out[-d] if i % 5 != g else out[-d] ^ int(rng.integers(1, 256)))

    for i, d in enumerate(order):
        c, per = counts[i], max(1, d // 5)
        if d == 1:
            out += _random(rng, 1, avoid=out[-1:])
            for v in rng.permutation(256)[:c].tolist():
                out += bytes([v]) * 4
        elif d < 256:
            while c > 0:
                out += _random(rng, -len(out) % 256 + 256)   # to a round's start, with a round of fresh bytes before it
                copy(d, min(per, c))
                c -= per
        else:
            c = int(c * 1.0004 ** d) + 1   # (about one window in 4096 / d has lost its place in the hash table by then)
            out += _random(rng, d)
            block = 0
            while c > 0:   # block after block, each the copy of the one before; the changed place moves on from block
                k = min(per, c)   # to block, so that no window with a changed byte in it stood there before
                copy(d, k, block % 5)
                out += _random(rng, d - 5 * k)
                c -= k
                block += 1
    assert len(out) <= MEMBER, len(out)
    return bytes(out)


def sweep():
    """name -> text: seeded families around what a DEFLATE encoder gets wrong.  tests/test_deflate_emulation.py holds
    the list (with texts()) to a census of the tokens it makes the compressor write."""
    rng = np.random.default_rng(1951)
    t = {}
    for p in PERIODS:
        n = max(3000, 2 * p + 700)
        t[f"period_{p}"] = (_random(rng, p) * (n // p + 1))[:n]
    # every match length: R[:L] again and again, each time one byte longer than the last copy
    R = _random(rng, 300)
    body = bytearray(R + _random(rng, 212))
    for L in range(3, 259):
        body += R[:L] + bytes([L & 0xFF, (L * 7 + 1) & 0xFF, (L >> 8) | 0x80])
    t["every_length"] = bytes(body)
    for d in DISTANCES:
        t[f"dist_{d}"] = _distance_text(rng, d)
    fq = fastq_like(rng, 1100)
    for n in range(1, 1101):
        t[f"len_{n}"] = fq[:n]
    t["two_symbols"] = bytes(rng.choice(list(b"AC"), size=MEMBER).astype(np.uint8))
    t["one_symbol_and_one"] = b"G" * (MEMBER - 1) + b"A"
    flat = np.repeat(np.arange(256, dtype=np.uint8), MEMBER // 256)
    rng.shuffle(flat)
    t["all_256_flat"] = flat.tobytes()
    t["skewed_with_matches"] = _skewed_with_matches()
    t["skewed_distances"] = _skewed_distances()
    # a 258-byte match from offset 254 / 255 of a round: the round after it holds no token start
    for at in (254, 255):
        t[f"covered_round_{at}"] = _random(rng, at - 1, avoid=b"X") + b"X" * 259 + _random(rng, 700, avoid=b"X")
    block = _random(rng, 300)
    t["covered_round_far"] = block + _random(rng, 1024 + 254 - 300) + block[:258] + _random(rng, 600)
    # fuzz: the six content kinds of test_gpu_inflate.test_inflate_fuzz_small_streams
    fq = fastq_like(rng, 200_000)
    for i in range(FUZZ):
        kind = int(rng.integers(0, 6))
        n = int(rng.integers(0, 70_001)) if i % 7 else int(rng.integers(0, 40))
        if kind == 0:
            x = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        elif kind == 1:
            x = rng.integers(65, 70, size=n, dtype=np.uint8).tobytes()
        elif kind == 2:
            o = int(rng.integers(0, len(fq) - n))
            x = fq[o:o + n]
        elif kind == 3:
            unit = rng.integers(0, 256, size=int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            x = (unit * (n // len(unit) + 1))[:n]
        elif kind == 4:
            x = bytes(rng.integers(0, 4, size=n, dtype=np.uint8) * 17 + 33)
        else:
            x = b"".join(b"%d\t%x\n" % (j * 7919 % 100003, j) for j in range(n // 12))
        t[f"fuzz_{i}"] = x
    return t


def gather_files():
    """40 files of 3..5 members of FASTQ-like text, 8.5 MB: the non-first members' places in their files have every
    residue mod 4 (tests/test_deflate_emulation.py holds them to that), which is what the gather kernel's lead bytes,
    realigned dwords and tail bytes depend on."""
    rng = np.random.default_rng(4004)
    pool = fastq_like(rng, 700_000)
    out = []
    for i in range(40):
        n = ((3, 4, 3, 5)[i % 4] - 1) * MEMBER + int(rng.integers(1, MEMBER + 1))
        o = int(rng.integers(0, len(pool) - n))
        out.append(pool[o:o + n])
    return out


SCAN_FILES, SCAN_SPARSE, SCAN_BLOCK = 9000, 4200, 4096


def scan_files():
    """9,000 files for one call whose two prefix sums (over members, over files) both take more than one block of 4,096:
    among the first 4,200 every third is empty (fewer members than files there), then one member a file, and one file
    of 5 members whose members lie on both sides of member 4096."""
    rng = np.random.default_rng(9006)   # (a seed with which no file around file 4096 ends on a multiple of 16)
    pool = fastq_like(rng, 5 * MEMBER)
    out = []
    members = 0
    for i in range(SCAN_FILES):
        if i < SCAN_SPARSE and i % 3 == 1:
            out.append(b"")
            continue
        if i >= SCAN_SPARSE and members == SCAN_BLOCK - 2:
            out.append(pool[:4 * MEMBER + 12345])
            members += 5
            continue
        n = int(rng.integers(1, 300))
        out.append(bytes(rng.choice(list(b"ACGTN\n@+I#"), size=n).astype(np.uint8)))
        members += 1
    return out


def check_scan_batch(texts, files=None):
    """The conditions of the scan test on its batch; with the compressed files, also that those around file 4096 do not
    end on a multiple of 16."""
    nmem = [-(-len(t) // MEMBER) for t in texts]
    assert len(texts) == SCAN_FILES and sum(nmem[:SCAN_SPARSE]) < SCAN_SPARSE and nmem[1:SCAN_SPARSE:3] == [0] * (SCAN_SPARSE // 3)
    assert SCAN_BLOCK < sum(nmem) < 10_000 and sum(nmem) != len(texts)
    big = nmem.index(5)
    assert nmem.count(5) == 1 and sum(nmem[:big]) < SCAN_BLOCK < sum(nmem[:big + 1])
    if files is not None:
        assert all(len(f) % 16 for f in files[SCAN_BLOCK - 8:SCAN_BLOCK + 8])


DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_sweep_sha256.json")


def digests(compress, named_files=None):
    """What tests/golden/deflate_sweep_sha256.json records, from `compress` (text -> file): name -> sha256 of the file
    for texts(), small_files(), sweep() and gather_files(), and one digest over all files of scan_files() one after
    another.  named_files: (name, text, file) already made for the first three."""
    if named_files is None:
        named = list(texts().items()) + [(f"small_{i}", t) for i, t in enumerate(small_files())] + list(sweep().items())
        named_files = [(name, t, compress(t)) for name, t in named]
    d = {name: hashlib.sha256(f).hexdigest() for name, _, f in named_files}
    for i, t in enumerate(gather_files()):
        d[f"gather_{i}"] = hashlib.sha256(compress(t)).hexdigest()
    scan = [compress(t) for t in scan_files()]
    check_scan_batch(scan_files(), scan)
    d["scan_batch"] = hashlib.sha256(b"".join(scan)).hexdigest()
    return d


def members_of(data):
    """The gzip members of a BGZF file as (whole member, its text), by the BC field's BSIZE; zlib inflates each."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert size <= 65536 and at + size <= len(data)
        m = data[at:at + size]
        d = zlib.decompressobj(31)
        text = d.decompress(m)
        assert d.eof and d.unused_data == b"", "BSIZE is not the member's size"
        assert struct.unpack_from("<II", m, size - 8) == (zlib.crc32(text), len(text))
        out.append((m, text))
        at += size
    return out


def huffman_only_size(text):
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(c.compress(text) + c.flush())


def bound(n):
    return -(-n // MEMBER) * 31 + n + 28


def check_file(name, text, data):
    """Every assertion on one compressed file that needs no engine."""
    import gzip
    assert gzip.decompress(data) == text, name
    mem = members_of(data)
    assert data.endswith(EOF) and mem[-1][0] == EOF, name
    assert b"".join(t for _, t in mem) == text, name
    assert len(mem) == -(-len(text) // MEMBER) + 1, name
    assert all(len(t) == MEMBER for _, t in mem[:-2]) and (len(mem) < 2 or 0 < len(mem[-2][1]) <= MEMBER), name
    assert len(data) <= bound(len(text)), name
    if text == b"":
        assert data == EOF
    if name.startswith("fastq_") or name in ("skewed", "repeated"):
        for m, t in mem[:-1]:
            assert len(m) <= huffman_only_size(t) + TABLE_ALLOWANCE + FRAMING, (name, len(m), huffman_only_size(t))
    if name == "repeated":   # (60,000 bytes: one member, and the matcher's check is asked of it)
        assert len(mem) == 2
        for m, t in mem[:-1]:
            assert 2 * len(m) < huffman_only_size(t), (name, len(m), huffman_only_size(t))
    if name == "far":
        # 3,000 of its random bytes can only be literals (the third thousand's source is one byte too far); the fourth
        # thousand is the match at distance 32,768 or another 1,000 bytes
        assert 3000 < len(data) < 3600, (name, len(data))
    if name == "random":
        assert len(data) == bound(len(text)), "the stored block"
