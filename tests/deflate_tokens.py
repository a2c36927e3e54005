"""A reader of DEFLATE blocks for the tests: which tokens a stream holds, not only what it inflates to.

Written from RFC 1951 (and RFC 1952 for a member's framing), in plain Python, without zlib and without a look at the
compressor under test.  zlib says "it inflates"; this says which block type, which code lengths, which literals and
which (length, distance) pairs were written, so that a set of test inputs can be held to conditions ("every length
symbol occurs").  tests/test_deflate_emulation.py proves it on zlib's own streams.

Fixed-Huffman blocks (BTYPE 1) are refused: the compressor writes none, and a census that met one would be wrong."""
from collections import namedtuple

# RFC 1951, 3.2.5
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]   # 3.2.7
FAST = 9   # bits of the first-level decoding table

Block = namedtuple("Block", "final btype hlit hdist ll_lengths d_lengths tokens")
Block.__doc__ = """One block.  btype 0 (stored): hlit = hdist = None, the tables empty, tokens are the literals.  btype 2:
hlit and hdist as the header states them (HLIT + 257 and HDIST + 1 are the tables' sizes).  tokens: (position, literal)
or (position, length, distance), position = offset of the token's first byte in the stream's text; the end-of-block
symbol is no token."""


def length_symbol(length):
    """The literal/length symbol (257..285) that states a match length (3..258)."""
    if length == 258:
        return 285
    return 257 + max(i for i in range(28) if LENGTH_BASE[i] <= length)


def distance_symbol(distance):
    return max(i for i in range(30) if DIST_BASE[i] <= distance)


class _Code:
    """A canonical Huffman code from its lengths (3.2.2); an index of the next FAST bits, bit by bit beyond."""

    def __init__(self, lengths):
        self.maxlen = max(lengths) if lengths else 0
        count = [0] * 16
        for n in lengths:
            count[n] += 1
        count[0] = 0
        nxt, code = [0] * 17, 0
        for n in range(1, 16):
            code = (code + count[n - 1]) << 1
            nxt[n] = code
        # a code may be incomplete (one distance code of one bit, 3.2.7) but never over-subscribed
        left = 1
        for n in range(1, 16):
            left = (left << 1) - count[n]
            if left < 0:
                raise ValueError("over-subscribed code")
        self.fast = [None] * (1 << FAST)
        self.slow = {}
        for sym, n in enumerate(lengths):
            if not n:
                continue
            c = nxt[n]
            nxt[n] += 1
            if n <= FAST:
                rev = int(format(c, "0%db" % n)[::-1], 2)
                for k in range(rev, 1 << FAST, 1 << n):
                    self.fast[k] = (sym, n)
            else:
                self.slow[(n, c)] = sym


class _Bits:
    def __init__(self, data, at):
        self.data, self.byte, self.acc, self.n = data, at, 0, 0

    def need(self, n):
        while self.n < n:
            if self.byte >= len(self.data):
                raise ValueError("the stream ends inside a block")
            self.acc |= self.data[self.byte] << self.n
            self.byte += 1
            self.n += 8

    def take(self, n):
        if n == 0:
            return 0
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.n -= n
        return v

    def to_byte(self):
        drop = self.n % 8
        self.acc >>= drop
        self.n -= drop

    def position(self):
        """the next unread byte, when the reader stands at a byte's start"""
        assert self.n % 8 == 0
        return self.byte - self.n // 8


def read_deflate(data, at=0):
    """The DEFLATE stream that starts at data[at]: (blocks, text, offset of the first byte behind the stream)."""
    b = _Bits(data, at)
    out = bytearray()
    blocks = []
    while True:
        final, btype = b.take(1), b.take(2)
        tokens = []
        if btype == 0:
            b.to_byte()
            n, nn = b.take(16), b.take(16)
            if n ^ nn != 0xFFFF:
                raise ValueError("stored block: LEN and NLEN disagree")
            for _ in range(n):
                tokens.append((len(out), b.take(8)))
                out.append(tokens[-1][1])
            blocks.append(Block(final, 0, None, None, [], [], tokens))
        elif btype == 2:
            hlit, hdist, hclen = b.take(5), b.take(5), b.take(4)
            cl = [0] * 19
            for i in range(hclen + 4):
                cl[CLEN_ORDER[i]] = b.take(3)
            clcode = _Code(cl)
            lengths = []
            while len(lengths) < hlit + 257 + hdist + 1:
                s = _symbol(b, clcode)
                if s < 16:
                    lengths.append(s)
                elif s == 16:
                    if not lengths:
                        raise ValueError("repeat without a length before it")
                    lengths += [lengths[-1]] * (3 + b.take(2))
                elif s == 17:
                    lengths += [0] * (3 + b.take(3))
                else:
                    lengths += [0] * (11 + b.take(7))
            if len(lengths) != hlit + 257 + hdist + 1:
                raise ValueError("a repeat runs over the tables' end")
            ll, dl = lengths[:hlit + 257], lengths[hlit + 257:]
            if ll[256] == 0:
                raise ValueError("no code for the end of block")
            llcode, dcode = _Code(ll), _Code(dl)
            # (the reader's state in local names for this loop: most of a census is spent here)
            fast, mask, data, size = llcode.fast, (1 << FAST) - 1, b.data, len(b.data)
            acc, n, byte, at = b.acc, b.n, b.byte, len(out)
            while True:
                while n < 48 and byte < size:
                    acc |= data[byte] << n
                    byte += 1
                    n += 8
                hit = fast[acc & mask]
                if hit is not None and hit[1] <= n:
                    s = hit[0]
                    acc >>= hit[1]
                    n -= hit[1]
                else:
                    b.acc, b.n, b.byte = acc, n, byte
                    s = _symbol(b, llcode)
                    acc, n, byte = b.acc, b.n, b.byte
                if s < 256:
                    tokens.append((at, s))
                    out.append(s)
                    at += 1
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise ValueError("length symbol 286 or 287")
                # at most 5 + 15 + 13 bits follow: they are in acc unless the stream ends
                b.acc, b.n, b.byte = acc, n, byte
                length = LENGTH_BASE[s - 257] + b.take(LENGTH_EXTRA[s - 257])
                d = _symbol(b, dcode)
                if d > 29:
                    raise ValueError("distance symbol 30 or 31")
                dist = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                acc, n, byte = b.acc, b.n, b.byte
                if dist > at:
                    raise ValueError("a distance reaches before the text's start")
                tokens.append((at, length, dist))
                if dist >= length:
                    out += out[at - dist:at - dist + length]
                else:
                    for _ in range(length):
                        out.append(out[-dist])
                at += length
            b.acc, b.n, b.byte = acc, n, byte
            blocks.append(Block(final, 2, hlit, hdist, ll, dl, tokens))
        else:
            raise ValueError("BTYPE %d is not read here" % btype)
        if final:
            break
    b.to_byte()
    return blocks, bytes(out), b.position()


def _symbol(b, code):
    """One symbol of a code: the table of FAST bits, or bit by bit."""
    while b.n < FAST and b.byte < len(b.data):
        b.acc |= b.data[b.byte] << b.n
        b.byte += 1
        b.n += 8
    hit = code.fast[b.acc & ((1 << FAST) - 1)]
    if hit is not None:
        if hit[1] > b.n:
            raise ValueError("the stream ends inside a code")
        b.acc >>= hit[1]
        b.n -= hit[1]
        return hit[0]
    # longer than FAST bits: the first FAST bits are no code, go on bit by bit
    c = 0
    for n in range(1, code.maxlen + 1):
        c = (c << 1) | b.take(1)
        if n > FAST and (n, c) in code.slow:
            return code.slow[(n, c)]
    raise ValueError("no such code")


def read_member(member):
    """One gzip member (RFC 1952) that holds ONE block, as a BGZF member does: (block, text).  The trailer is left
    to the caller's judge."""
    if member[:3] != b"\x1f\x8b\x08":
        raise ValueError("no gzip member")
    flg, at = member[3], 10
    if flg & 4:
        at += 2 + (member[at] | member[at + 1] << 8)
    for bit in (8, 16):
        if flg & bit:
            at = member.index(b"\0", at) + 1
    if flg & 2:
        at += 2
    blocks, text, end = read_deflate(member, at)
    if len(blocks) != 1 or end + 8 != len(member):
        raise ValueError("not one block and a trailer")
    return blocks[0], text
