"""The texts that the BGZF compressor's tests share (tests/test_gpu_deflate.py on the GPU, tests/test_deflate_emulation.py
on the host emulation) and what every compressed file must satisfy.  zlib is the judge, never the code under test."""
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
