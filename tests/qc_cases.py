"""Named cases of `--qc-report` (tests/qc_ref.py is the rule): each a list of streams (text, records).  The rule tests
hold the two statements of the rule to each other on them, the emulation runs the lane-local device code on them, the GPU
tests hold vk_qc_device to the rule.  Nothing here is larger than the carry case (5.5 MB)."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name streams")   # streams: [(text bytes, record budget)]

BASES = b"ACGTNacgtRY"
SWEEP_LENGTHS = (list(range(0, 131)) + [191, 192, 193, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 20000])


def sweep_record(ls, name=b"r"):
    """A record of ls bases: quality (7 c + ls) mod 94 at cycle c, bases cycling through ACGTNacgtRY -- a wrong cycle or a
    wrong class shows."""
    c = np.arange(ls)
    seq = np.frombuffer(BASES, dtype=np.uint8)[c % len(BASES)].tobytes()
    qual = (33 + (7 * c + ls) % 94).astype(np.uint8).tobytes()
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def length_sweep():
    text = b"".join(sweep_record(ls, b"len%d" % ls) for ls in SWEEP_LENGTHS)
    return Case("length_sweep", [(text, len(SWEEP_LENGTHS))])


def framing():
    plain = sweep_record(40, b"a") + sweep_record(75, b"b") + sweep_record(3, b"c")
    crlf = plain.replace(b"\n", b"\r\n")
    named = plain.replace(b"\n+\n", b"\n+a name\n")
    no_final = plain[:-1]
    no_final_crlf = crlf[:-1]          # (ends with \r: the last line's \r is no part of it)
    qual_at = b"@q1\nACGT\n+\n@III\n@q2\nACGTA\n+q2\n+IIII\n@q3\nAC\n+\n@+\n"
    odd_bytes = b"@o\nACGTACGT\n+\n I\x7fI\xffI !\n@p\nAC\n+\n\x7f\xff"
    ragged = (b"@s\nACGTACGT\n+\nIIIIIII\n" + sweep_record(20, b"ok") + b"@l\nACGTACGT\n+\nIIIIIIIII\n" +
              b"@e\n\n+\nI\n" + b"@f\nA\n+\n\n")
    only_ragged = b"@s\nACGT\n+\nIII\n"
    streams = [plain, crlf, named, no_final, no_final_crlf, qual_at, odd_bytes, ragged, only_ragged, b""]
    return Case("framing", [(t, (t.count(b"\n") + (1 if t and not t.endswith(b"\n") else 0)) // 4) for t in streams])


def budgets():
    recs = [sweep_record(30 + (i * 7) % 50, b"b%d" % i) for i in range(130)]
    text = b"".join(recs)
    streams = [(text, n) for n in (0, 1, 129, 130, 131)]
    bad_header = b"".join(recs[:2]) + b"#" + recs[2][1:] + b"".join(recs[3:])
    bad_plus = b"".join(recs[:2]) + recs[2].replace(b"\n+\n", b"\n-\n", 1) + b"".join(recs[3:])
    empty_plus = b"".join(recs[:2]) + recs[2].replace(b"\n+\n", b"\n\n", 1) + b"".join(recs[3:])
    for t in (bad_header, bad_plus, empty_plus):
        streams += [(t, 130), (t, 3), (t, 2)]   # the defect inside the budget twice, then behind it
    short = text[:len(text) - len(recs[-1]) // 2]   # (the last record cut inside its sequence line: 518 lines)
    streams += [(short, 130), (short, 129)]
    return Case("budgets", streams)


def many_streams():
    rng = np.random.default_rng(20251020)
    streams = []
    for i in range(300):
        n = int(rng.integers(0, 4))
        text = b"".join(sweep_record(0 if rng.integers(0, 5) == 0 else int(rng.integers(1, 200)), b"s%d_%d" % (i, j)) for j in range(n))
        if n and i % 7 == 3:
            text = text[:-1]   # (no final newline: what follows the stream must not be taken for its quality line)
        streams.append((text, n))
    return Case("many_streams", streams)


def carry():
    rec = b"@c\n" + b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT" + b"\n+\n" + b"~" * 36 + b"\n"
    return Case("carry", [(rec * 70000, 70000)])


CASES = (length_sweep, framing, budgets, many_streams, carry)


def all_cases():
    return [make() for make in CASES]


GAP = b"IIII\n@gap\nACGT\n+\nIIII\n#"   # what lies between two streams: bytes that no stream may count


def pack(streams):
    """The streams laid out as vk_qc_device takes them: (buffer uint8, offsets, lengths, records) -- every stream at a
    multiple of 16 bytes, GAP's bytes right behind its end up to the next stream, the buffer readable 16 bytes past the
    last stream's rounded end."""
    offs, lens, recs, parts, at = [], [], [], [], 0
    for text, n in streams:
        offs.append(at)
        lens.append(len(text))
        recs.append(n)
        room = (len(text) + 15) // 16 * 16 + 16 - len(text)
        parts.append(text + (GAP * 2)[:room])
        at += len(text) + room
    buf = np.frombuffer(b"".join(parts) + b"\0" * 16, dtype=np.uint8)
    return (buf, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64), np.array(recs, dtype=np.uint64))
