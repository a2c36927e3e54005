"""The rule of step C's files (`image --write-splits`) restated in plain Python: the contract the GPU's
vk_ladder_emit_device must meet byte for byte ("Step C").  Written from the rule, one record at a
time; plus the inputs the CPU and GPU tests share.  Tests only."""
import random

BREAK = 500                      # reformat.sh's breaklength (commands/image.py:586-588)
BASES = frozenset(b"ACGTacgt")


def sample_hash(seed, anchor):
    """oracle/vk_oracle.c's vko_sample_hash, restated."""
    m = 0xFFFFFFFF
    h = (anchor ^ seed) & m
    h = (h + ((anchor >> 32) * 0x9E3779B1 & m) + (seed >> 32)) & m
    h ^= h >> 16
    h = h * 0x85EBCA6B & m
    h ^= h >> 13
    h = h * 0xC2B2AE35 & m
    h ^= h >> 16
    return h


def framing_status(text):
    """The status bits the read index gives a sample: 1 the text does not start with '@' or its third line not with
    '+'; 2 its lines (a last one without newline counted) are no multiple of 4."""
    if not text:
        return 0
    st = 0
    if text[:1] != b"@":
        st |= 1
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    if len(lines) > 2 and lines[2][:1] != b"+":
        st |= 1
    if len(lines) % 4:
        st |= 2
    return st


def records(text):
    """(anchor, header, sequence, quality) of every record: lines 4 r .. 4 r + 3, each without its trailing '\\r'; the
    anchor is the offset of the newline that ends the header line."""
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    out, pos = [], 0
    for r in range(len(lines) // 4):
        h, s, p, q = lines[4 * r:4 * r + 4]
        anchor = pos + len(h)
        pos += len(h) + len(s) + len(p) + len(q) + 4
        out.append((anchor,) + tuple(x[:-1] if x.endswith(b"\r") else x for x in (h, s, q)))
    return out


def emit_ref(text, seed, threshold, whole=False):
    """The file of one ladder step.  Sampled (whole=False): the records with sample_hash(seed, anchor) < threshold, a
    read of more than 500 bases as records of 500 named `<header>_<n>`; whole: every record, uncut.  Bad framing:
    nothing."""
    if framing_status(text):
        return b""
    out = []
    for anchor, h, s, q in records(text):
        if not whole and not sample_hash(seed, anchor) < threshold:
            continue
        s = bytes(b if b in BASES else ord("N") for b in s)
        if whole or len(s) <= BREAK:
            out.append(h + b"\n" + s + b"\n+\n" + q + b"\n")
            continue
        for n, a in enumerate(range(0, len(s), BREAK)):
            piece = s[a:a + BREAK]   # (the quality: the same byte range of its line, as far as the line goes)
            out.append(h + b"_" + str(n + 1).encode() + b"\n" + piece + b"\n+\n" + q[a:a + len(piece)] + b"\n")
    return b"".join(out)


def emitted_bases(text):
    """Bytes of the sequence lines of emitted text (every line ends in '\\n')."""
    return sum(len(x) for x in text.split(b"\n")[1::4])


# ------------------------------------------------------------------ inputs --

def _read(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _fastq(reads, eol="\n", plus="+", last_newline=True, qual=None):
    parts = []
    for i, (name, seq) in enumerate(reads):
        q = qual(i, seq) if qual else "".join(chr(33 + (j * 7 + i) % 41) for j in range(len(seq)))
        parts.append(f"@{name}{eol}{seq}{eol}{plus if not callable(plus) else plus(i)}{eol}{q}{eol}")
    text = "".join(parts).encode("latin-1")
    return text if last_newline else text[:-len(eol)]


def lengths_for(k):
    """Read lengths that put windows on both sides of every cut."""
    return [0, k - 1, k, 499, 500, 501, 1000, 1001, 1499 + k]


def case_inputs(k):
    """{name: FASTQ text} for window size k: a few KB each."""
    rng = random.Random(1000 + k)
    lens = lengths_for(k)
    plain = [(f"r{i}.{n}", _read(rng, n)) for i, n in enumerate(lens * 2)]
    cases = {"lengths": _fastq(plain)}
    cases["crlf"] = _fastq(plain, eol="\r\n")
    cases["plus_name"] = _fastq(plain, plus=lambda i: "+r%d" % i)
    cases["no_last_newline"] = _fastq(plain[:7], last_newline=False)
    cases["crlf_no_last_newline"] = _fastq(plain[:7], eol="\r\n", last_newline=False)
    mixed = [(f"m{i}", _read(rng, n, "ACGTacgtNnRYKMSWBDHV.-*")) for i, n in enumerate([40, 150, 501, 1200, 3, 700])]
    cases["lower_iupac"] = _fastq(mixed)
    nrun = []
    for i, (a, b) in enumerate([(495, 10), (990, 20), (500, 1), (499, 1), (1498, 4)]):   # N runs across multiples of 500
        nrun.append((f"n{i}", _read(rng, a) + "N" * b + _read(rng, 300)))
    cases["n_runs"] = _fastq(nrun)
    cases["long_header"] = _fastq([("h0 " + "x" * 20000, _read(rng, 1200)), ("h1", _read(rng, 90)),
                                   ("h2 " + "y" * 700, _read(rng, 501))])
    cases["short_quality"] = _fastq([("q0", _read(rng, 1300)), ("q1", _read(rng, 200)), ("q2", _read(rng, 800))],
                                    qual=lambda i, seq: "I" * [600, 0, 1000][i])
    return cases


SEEDS = (0, 7)
THRESHOLDS = (0, 1, 1 << 31, (1 << 32) - 1, 1 << 32)
