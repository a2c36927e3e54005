"""Step B inputs at the places the hand cases and synth_set never reach: read budgets that end inside a file, bytes
behind a file's end, lines longer than a 16 KiB newline chunk, more than 2^20 units (the scan's second round), hundreds
of samples and files, dirty and asymmetric pairs, and FASTQ framing that is unusual but well-formed.  Seeded builders
that the CPU tests (test_clean_rules.py) and the GPU tests (test_gpu_clean_edges.py) share.

A builder returns a *batch*: dict(texts, roles, owner, records, nsamples[, slack]) -- file i gives its first
records[i] records to sample owner[i] as roles[i] (0 single reads, 1 R1, 2 R2: the VK_CL_ROLE_* values); slack[i] is
what lies in device memory right behind file i's end (past its length, so it must never be read as text).
expected() states what vk_clean_device must give for a batch, with nothing but clean_ref.  Tests only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_ref as R  # noqa: E402

SE, R1, R2 = 0, 1, 2                 # VK_CL_ROLE_UNPAIRED / _R1 / _R2
BAD_FRAMING, RAGGED = 1, 2           # VK_CL_BAD_FRAMING / VK_CL_RAGGED
NSTAT = 2 + 5 * R.CYCLES             # clean_bp, records, base[40][4], reach[40]
CHUNK = 16384                        # bytes of a newline-pass workgroup (kClChunk)
FLAGS = [(a, m, d) for a in (True, False) for m in (True, False) for d in (True, False)]
TRIMS = [(0, 0), (10, 10), (7, 3)]
GARBAGE = b"no at sign\nACGT\n+\nIIII\n@wrong plus\nACGT\n-\nIIII\n@short quality\nACGTACGT\n+\nIII\n"


class Batch(dict):
    """A batch under construction: add(text, role, sample, budget) -> the file's index."""

    def __init__(self):
        super().__init__(texts=[], roles=[], owner=[], records=[], nsamples=0)

    def add(self, text, role, sample, budget=None):
        self["texts"].append(text)
        self["roles"].append(role)
        self["owner"].append(sample)
        self["records"].append(text.count(b"\n") // 4 if budget is None else budget)
        self["nsamples"] = max(self["nsamples"], sample + 1)
        return len(self["texts"]) - 1

    def add_sample(self, r1, r2, se):
        """A sample of whole files, one per group that has records; its index."""
        j = self["nsamples"]
        self["nsamples"] += 1
        for recs, role in ((se, SE), (r1, R1), (r2, R2)):
            if recs:
                self.add(R.fq(recs), role, j)
        return j


def stats_words(st):
    """The VK_CL_NSTAT words of a clean_sample stats dict."""
    return [st["clean_bp"], st["records"]] + [v for row in st["base"] for v in row] + list(st["reach"])


def groups(batch):
    """Per sample (r1, r2, singles, status): the budgeted records of its files, concatenated per group in file order;
    RAGGED iff the R1 and R2 budgets sum differently, BAD_FRAMING iff a file's budgeted records do not parse."""
    out = [([], [], [], 0) for _ in range(batch["nsamples"])]
    want = [[0, 0, 0] for _ in range(batch["nsamples"])]
    for text, role, j, n in zip(batch["texts"], batch["roles"], batch["owner"], batch["records"]):
        r1, r2, se, status = out[j]
        recs = R.parse_fastq(text, n)
        want[j][role] += n
        if recs is None:
            status |= BAD_FRAMING
        else:
            (se, r1, r2)[role].extend(recs)
        out[j] = (r1, r2, se, status)
    return [(r1, r2, se, status | (RAGGED if w[R1] != w[R2] else 0)) for (r1, r2, se, status), w in zip(out, want)]


def expected(batch, F=10, T=10, adapter=True, merge=True, dedup=True):
    """[(text, stats words, status)] per sample.  A flagged sample has no text and no stats.  A batch's "closed"
    entries {sample: fn(F, T, adapter, merge, dedup) -> (text, words)} state a sample in closed form."""
    out = []
    for j, (r1, r2, se, status) in enumerate(groups(batch)):
        if status:
            out.append((b"", [0] * NSTAT, status))
        elif j in batch.get("closed", {}):
            out.append(batch["closed"][j](F, T, adapter, merge, dedup) + (0,))
        else:
            text, st = R.clean_sample(r1, r2, se, F=F, T=T, adapter=adapter, merge=merge, dedup=dedup)
            out.append((text, stats_words(st), 0))
    return out


def _reads(rng, n, tag, lo=20, hi=120):
    """n single-end records of lo..hi random bases."""
    out = []
    for i in range(n):
        k = int(rng.integers(lo, hi + 1))
        out.append((b"@%s%d" % (tag, i), R._rng_seq(rng, k), R._qual(rng, k)))
    return out


def _fill_to(rng, nbytes, tag, L=100):
    """Records whose FASTQ text is exactly nbytes long (nbytes >= 3 records)."""
    recs, left = [], nbytes
    i = 0
    while True:
        h = b"@%s%04d" % (tag, i)
        size = len(h) + 2 * L + 5
        if left >= 2 * size + 16:
            recs.append((h, R._rng_seq(rng, L), R._qual(rng, L)))
            left -= size
            i += 1
            continue
        # two records take what is left: an even number of sequence bytes in each
        a = (left // 2 - len(h) - 5) // 2
        recs.append((h, R._rng_seq(rng, a), R._qual(rng, a)))
        left -= len(h) + 2 * a + 5
        h = b"@%s%04d" % (tag, i + 1)
        if (left - len(h) - 5) % 2:
            h += b"x"
        b = (left - len(h) - 5) // 2
        recs.append((h, R._rng_seq(rng, b), R._qual(rng, b)))
        assert len(R.fq(recs)) == nbytes
        return recs


# ------------------------------------------------------------------ budgets ---

def budgets():
    """Budgets that end inside files.  Returns the batch with "names": {what: sample}."""
    rng = np.random.default_rng(301)
    b = Batch()
    names = {}
    r1, r2, se = R.synth_set(302, 400, 120, L=101)
    extra = _reads(rng, 60, b"extra")
    # 0: two R1 and two R2 files of different sizes, split at 150 and at 260, unbudgeted records behind three of
    # them; the single reads in three files, the middle one with budget 0
    names["crossed"] = 0
    b.add(R.fq(r1[:150] + extra[:30]), R1, 0, 150)
    b.add(R.fq(r1[150:] + extra[30:35]), R1, 0, 250)
    b.add(R.fq(r2[:260] + extra[35:42]), R2, 0, 260)
    b.add(R.fq(r2[260:]), R2, 0, 140)
    b.add(R.fq(se[:50]), SE, 0, 50)
    b.add(R.fq(extra[42:]), SE, 0, 0)
    b.add(R.fq(se[50:] + extra[:9]), SE, 0, 70)
    # 1: every budget 0
    names["all_zero"] = 1
    p1, p2, ps = R.synth_set(303, 30, 20, L=80)
    b.add(R.fq(p1), R1, 1, 0)
    b.add(R.fq(p2), R2, 1, 0)
    b.add(R.fq(ps), SE, 1, 0)
    # 2: one record of a single-end file
    names["one"] = 2
    b.add(R.fq(_reads(rng, 25, b"one")), SE, 2, 1)
    # 3 / 4: a budget that ends with a chunk's last byte, and one record later
    b["chunk_files"] = {}
    for j, (tag, more) in enumerate(((b"at", 0), (b"past", 1))):
        full = _fill_to(rng, CHUNK, tag)
        names["chunk_" + tag.decode()] = 3 + j
        i = b.add(R.fq(full + _reads(rng, 20, tag)), SE, 3 + j, len(full) + more)
        b["chunk_files"][tag.decode()] = (i, len(full))
    # 5: garbage behind the budget, as single reads and behind R2
    names["garbage"] = 5
    g1, g2, gs = R.synth_set(304, 40, 40, L=90)
    b.add(R.fq(g1), R1, 5, 40)
    names["garbage_file"] = b.add(R.fq(g2) + GARBAGE, R2, 5, 40)
    b.add(R.fq(gs) + GARBAGE, SE, 5, 40)
    # 6: files of equal size, budgets 30 and 29
    names["ragged"] = 6
    q1, q2, _ = R.synth_set(305, 30, 0, L=70)
    b.add(R.fq(q1), R1, 6, 30)
    b.add(R.fq(q2), R2, 6, 29)
    # 7: an ordinary sample behind them
    names["plain"] = b.add_sample(*R.synth_set(306, 50, 30, L=75))
    b["names"] = names
    return b


# ---------------------------------------------------------------- file ends ---

SLACK_RECORD = b"@\n\n+\n\n"       # a complete record, four newlines in six bytes


def file_ends():
    """Single-read files of every length modulo 64, of 16383 / 16384 / 16385 bytes, without a final newline, of no
    bytes; each with at least 80 bytes of well-formed records behind its end that are no part of it."""
    rng = np.random.default_rng(401)
    b = Batch()
    for r in range(64):
        recs = _reads(rng, int(rng.integers(2, 7)), b"e%d_" % r, 10, 70)
        h, s, q = recs[-1]
        recs[-1] = (h + b"." * ((r - len(R.fq(recs))) % 64), s, q)
        b.add(R.fq(recs), SE, b["nsamples"])
    b["sized"] = {}
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):
        b["sized"][n] = b.add(R.fq(_fill_to(rng, n, b"z")), SE, b["nsamples"])
    recs = _reads(rng, 9, b"cut")
    b["unterminated"] = b.add(R.fq(recs)[:-1], SE, b["nsamples"])
    b["empty"] = b.add(b"", SE, b["nsamples"])
    j = b["nsamples"]                    # an empty file between two others of a group
    b.add(R.fq(_reads(rng, 5, b"m")), SE, j)
    b.add(b"", SE, j)
    b.add(R.fq(_reads(rng, 4, b"n")), SE, j)
    b["slack"] = [SLACK_RECORD * (14 + i % 5) for i in range(len(b["texts"]))]
    return b


# --------------------------------------------------------------- long lines ---

def long_lines():
    """A 40,000-base read under a 20,000-byte header and a pair of 20,000-base mates that overlap, among ordinary
    reads: chunks without a newline, records that start anywhere in a chunk."""
    rng = np.random.default_rng(501)
    b = Batch()
    big = (b"@long " + b"h" * 19994, R._rng_seq(rng, 40000), R._qual(rng, 40000))
    b.add_sample([], [], _reads(rng, 70, b"a") + [big] + _reads(rng, 90, b"b"))
    r1, r2, _ = R.synth_set(502, 120, 0, L=110)
    a, c = R.pair_from_insert(rng, b"mates", R._rng_seq(rng, 31000), 20000)
    b.add_sample(r1[:47] + [a] + r1[47:], r2[:47] + [c] + r2[47:], _reads(rng, 30, b"c"))
    return b


# --------------------------------------------------------------- many small ---

UNIT_CYCLE = (0, 1, 2, 3, 5, 15, 16, 17, 63, 64, 65)
ADAPTERS = (b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT", b"CTGTCTCTTATACACATCT")


def many_small(n=300, seed=601):
    """n samples of UNIT_CYCLE[j % 11] units, pairs only / single reads only / both in turn (every sample keeps the
    files of its kind, empty ones too): sample boundaries at every kind of position of a 64-unit and a 256-unit
    workgroup.  A part of the reads runs into an adapter (short inserts that the overlap cannot see, single reads
    that read through), so that trimming by sequence has work in every sample."""
    rng = np.random.default_rng(seed)
    b = Batch()
    L = 80
    for j in range(n):
        units, kind = UNIT_CYCLE[j % len(UNIT_CYCLE)], j % 3
        npairs = units if kind == 0 else 0 if kind == 1 else units // 2
        r1, r2, se = [], [], []
        for p in range(npairs):
            x = rng.random()
            lo, hi = (8, 30) if x < 0.3 else (40, L) if x < 0.6 else (L, 2 * L)
            ins = R._rng_seq(rng, int(rng.integers(lo, hi)))
            a, c = R.pair_from_insert(rng, b"s%dp%d" % (j, p), ins, L, ADAPTERS[j % 3], ADAPTERS[(j + 1) % 3])
            r1.append(a)
            r2.append(c)
        for s in range(units - npairs):
            if rng.random() < 0.4:
                seq = (R._rng_seq(rng, int(rng.integers(15, 60))) + ADAPTERS[(j + 2) % 3] + b"G" * L)[:L]
            else:
                seq = R._rng_seq(rng, int(rng.integers(1, L + 1)))
            se.append((b"@s%ds%d" % (j, s), seq, R._qual(rng, len(seq))))
        if kind != 1:
            b.add(R.fq(r1), R1, j)
            b.add(R.fq(r2), R2, j)
        if kind != 0:
            b.add(R.fq(se), SE, j)
        b["nsamples"] = j + 1
    b["adapters"] = [[ADAPTERS[j % 3], ADAPTERS[(j + 1) % 3], ADAPTERS[(j + 2) % 3]] for j in range(n)]
    return b


# -------------------------------------------------------------- dirty pairs ---

KEPT = (0, 1, 29, 30, 31, 49, 50, 51, 150)
_OTHER = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
_IUPAC_PAIR = {ord("R"): ord("Y"), ord("Y"): ord("R"), ord("."): ord("."), ord("-"): ord("-")}


def _dirty(rng, seq, alphabet):
    s = bytearray(seq)
    if alphabet == 1:
        for i in np.flatnonzero(rng.random(len(s)) < 0.05):
            s[i] = ord("N")
    elif alphabet == 2:
        for i in np.flatnonzero(rng.random(len(s)) < 0.04):
            s[i] |= 0x20
    elif alphabet == 3:
        for i in np.flatnonzero(rng.random(len(s)) < 0.03):
            s[i] = b"RY.-"[int(rng.integers(0, 4))]
    return bytes(s)


def dirty_pairs(F=10, T=10, n=3000, seed=701):
    """About n pairs as records (r1, r2) in one sample, for the trim (F, T): mates of KEPT[..] + F + T bases each on
    its own (and a few shorter than F + T), inserts shorter than, equal to and longer than the reads, four alphabets,
    4 / 5 / 6 mismatches planted among the first 50 compared positions, equal and unequal non-ACGT bytes facing each
    other there, duplicates and pairs that differ in R2 alone."""
    rng = np.random.default_rng(seed + 16 * F + T)
    full = 150 + F + T
    r1, r2 = [], []

    def put(name, a, c):
        r1.append((b"@" + name + b" 1", a, R._qual(rng, len(a))))
        r2.append((b"@" + name + b" 2", c, R._qual(rng, len(c))))

    for p in range(n):
        x = rng.random()
        if p > 10 and x < 0.1:                       # an exact duplicate (names and qualities differ)
            j = int(rng.integers(0, p))
            put(b"dup%d" % p, r1[j][1], r2[j][1])
            continue
        if p > 10 and x < 0.2:                       # R1 of an earlier pair, its R2 with one base changed
            j = int(rng.integers(0, p))
            c = bytearray(r2[j][1])
            if c:
                i = int(rng.integers(0, len(c)))
                c[i] = _OTHER.get(c[i], b"A")[0]
            put(b"r2only%d" % p, r1[j][1], bytes(c))
            continue
        if x < 0.45:                                 # full-length mates with planted mismatches (and facing bytes)
            ins = R._rng_seq(rng, int(rng.integers(60 + F + T, 240 + F + T)))
            (_, a, _), (_, c, _) = R.pair_from_insert(rng, b"", ins, full)
            a, c = bytearray(a), bytearray(c)
            k = F - (len(ins) - full + T)            # backward by k (> 0) or forward by -k
            pos = rng.permutation(50)
            m = (4, 5, 6)[p % 3]
            for i in pos[:m]:
                y = full - T - 1 - max(0, k) - int(i)
                c[y] = _OTHER[c[y]][0]
            facing = (p // 3) % 4                    # 0 none, 1 N / N, 2 n / N, 3 R / Y
            if facing:
                i = int(pos[m])
                y = full - T - 1 - max(0, k) - i
                z = F + max(0, -k) + i
                a[z], c[y] = {1: b"NN", 2: b"nN", 3: b"RY"}[facing]
            put(b"m%d_f%d_%d" % (m, facing, p), bytes(a), bytes(c))
            continue
        # mates of independent lengths, any insert, one of four alphabets
        if rng.random() < 0.08 and F + T:
            l1, l2 = int(rng.integers(0, F + T)), int(rng.integers(0, full + 1))
        else:
            l1, l2 = (int(KEPT[rng.integers(0, len(KEPT))]) + F + T for _ in range(2))
        if rng.random() < 0.5:
            l1, l2 = l2, l1
        Lm = max(l1, l2, 1)
        kind = rng.random()
        nins = int(rng.integers(max(1, Lm - 60), Lm)) if kind < 0.35 and Lm > 1 else Lm if kind < 0.45 else \
            int(rng.integers(Lm + 1, 2 * Lm + 40))
        alphabet = int(rng.integers(0, 4))
        ins = _dirty(rng, R._rng_seq(rng, nins), alphabet)
        (_, a, _), (_, c, _) = R.pair_from_insert(rng, b"", ins, Lm)
        if alphabet == 2:                            # R2 is read on its own: its own lower case
            c = _dirty(rng, c, 2)
        elif alphabet == 3:                          # ... and the complement of R1's byte where R1 has no base, not N
            c = bytes(_IUPAC_PAIR.get(ins[len(ins) - 1 - y], ch) if y < len(ins) else ch for y, ch in enumerate(c))
        put(b"k%d_%d_a%d_%d" % (l1, l2, alphabet, p), a[:l1], c[:l2])
    b = Batch()
    b.add_sample(r1, r2, [])
    b["pairs"] = (r1, r2)
    return b


def outcome(a, c, F, T):
    """What the rules make of the pair (a, c) alone with every flag on: "dropped" (nothing written), "merged",
    "cut" (the overlap cut adapters; whatever happened after) or "unmerged"; "cut" wins over "merged"."""
    ta, tc = R._trim(a, F, T), R._trim(c, F, T)
    text, _ = R.clean_sample([a], [c], [], F=F, T=T)
    if not text:
        return "dropped"
    ov = R.overlap(ta[1], tc[1])
    if ov is not None and ov[0] < 0:
        return "cut"
    return "merged" if text.count(b"\n") == 4 and ov is not None else "unmerged"


# ------------------------------------------------------------------ framing ---

def _text(records, eol=b"\n"):
    """FASTQ text of (header, seq, third line, qual)."""
    return b"".join(h + eol + s + eol + p + eol + q + eol for h, s, p, q in records)


def _odd(recs):
    """The records with the unusual but well-formed shapes among them, as (header, seq, third line, qual)."""
    out = []
    for i, (h, s, q) in enumerate(recs):
        k = i % 7
        if k == 0:
            out.append((h, s, b"+" + h[1:], q))                  # +name
        elif k == 1 and s:
            out.append((h, s, b"+", b"@" + q[1:]))               # quality that starts with '@'
        elif k == 2 and s:
            out.append((h, s, b"+", b"+" + q[1:]))               # ... with '+'
        elif k == 3:
            out.append((b"@", s, b"+", q))                       # a header that is just '@'
        elif k == 4:
            out.append((h, b"", b"+", b""))                      # no bases
        elif k == 5 and s:
            out.append((h, s, b"+" + h[1:], b"@+"[i % 2:][:1] + q[1:]))
        else:
            out.append((h, s, b"+", q))
    return out


def framing():
    """CRLF files and the odd shapes of _odd, each as single reads and as pairs; all well-formed."""
    b = Batch()
    r1, r2, se = R.synth_set(802, 150, 150, L=90)
    b.add(_text([(h, s, b"+", q) for h, s, q in se], b"\r\n"), SE, 0)
    b.add(_text([(h, s, b"+", q) for h, s, q in r1], b"\r\n"), R1, 1)
    b.add(_text([(h, s, b"+", q) for h, s, q in r2], b"\r\n"), R2, 1)
    r1, r2, se = R.synth_set(803, 150, 150, L=90)
    b.add(_text(_odd(se)), SE, 2)
    b.add(_text(_odd(r1)), R1, 3)
    b.add(_text(_odd(r2[3:] + r2[:3])), R2, 3)    # (shifted: a pair's mates take different shapes)
    return b


# ------------------------------------------------------------- big identity ---

def big_identity(n=1_100_000):
    """One single-read sample of n records of 62 bytes ('@r' + 7 digits, 24 bases over A C T, '+', 24 qualities) whose
    first 14 bases are the ordinal in base 3, then a small ordinary sample.  More than 2^20 units: the scan of the
    output bytes takes a second round at its top.  No read has a G, all differ, so with F = T = 0 the cleaned text is
    the input under every flag combination, and the stats follow from the columns."""
    assert n < 3 ** 14 and n < 10 ** 7
    rng = np.random.default_rng(901)
    idx = np.arange(n, dtype=np.int64)
    rec = np.empty((n, 62), dtype=np.uint8)
    rec[:, 0], rec[:, 1] = ord("@"), ord("r")
    for d in range(7):
        rec[:, 2 + d] = ord("0") + (idx // 10 ** (6 - d)) % 10
    act = np.frombuffer(b"ACT", dtype=np.uint8)
    for d in range(14):
        rec[:, 10 + d] = act[(idx // 3 ** (13 - d)) % 3]
    rec[:, 24:34] = act[rng.integers(0, 3, (n, 10))]
    rec[:, 9] = rec[:, 34] = rec[:, 36] = rec[:, 61] = ord("\n")
    rec[:, 35] = ord("+")
    rec[:, 37:61] = rng.integers(33, 74, (n, 24), dtype=np.uint8)
    text = rec.tobytes()
    seq = rec[:, 10:34]
    words = [24 * n, n]
    for c in range(R.CYCLES):
        words += [int((seq[:, c] == ch).sum()) if c < 24 else 0 for ch in b"ACGT"]
    words += [n if c < 24 else 0 for c in range(R.CYCLES)]

    def closed(F, T, adapter, merge, dedup):
        assert F == 0 and T == 0
        return text, words

    b = Batch()
    b.add(text, SE, 0)
    b.add_sample(*R.synth_set(902, 200, 100, L=60))
    b["closed"] = {0: closed}
    return b
