"""The cleaning rules of step B (`image --from-raw`) restated in plain Python: the contract the GPU's
vk_clean_device must meet byte for byte ("Step B").  Written from the rules, one read at a time
(only the overlap search is vectorised, over offsets); plus the hand cases and the seeded synthetic sets the CPU and
GPU tests share.  Tests only."""
import gzip

CYCLES = 40


def parse_fastq(text, nrec=None):
    """The first `nrec` records (None: all) of FASTQ text as (header line, sequence, quality) byte strings.  A file
    holds `newlines // 4` records (`wc -l`, then islice of 4 n lines).  None when a record taken is malformed."""
    lines = text.split(b"\n")
    n = text.count(b"\n") // 4
    if nrec is not None:
        if nrec > n:
            return None
        n = nrec
    out = []
    for r in range(n):
        h, s, p, q = lines[4 * r:4 * r + 4]
        if not h.startswith(b"@") or not p.startswith(b"+") or len(q) != len(s):
            return None
        out.append((h, s, q))
    return out


def read_text(path):
    with open(path, "rb") as f:
        head = f.read(2)
    if head == b"\x1f\x8b":
        with gzip.open(path, "rb") as f:
            return f.read()
    with open(path, "rb") as f:
        return f.read()


_COMP = {ord("A"): "T", ord("a"): "T", ord("T"): "A", ord("t"): "A", ord("C"): "G", ord("c"): "G", ord("G"): "C",
         ord("g"): "C"}


def revcomp(seq):
    """fastp's reverse complement: A C G T in either case to the upper-case complement, anything else to N."""
    return bytes(ord(_COMP.get(b, "N")) for b in reversed(seq))


def poly_g(seq):
    """Length after fastp's poly-G tail trim (min length 10)."""
    n = len(seq)
    mism, first_g, i = 0, n - 1, 0
    broke = False
    for i in range(n):
        if seq[n - 1 - i] != ord("G"):
            mism += 1
        else:
            first_g = n - 1 - i
        if mism > 5 or (mism > (i + 1) // 8 and i >= 9):
            broke = True
            break
    if not broke:
        i = n
    return first_g if i >= 10 else n


def overlap(s1, r2):
    """(off, ol) of the first accepted offset between s1 and the reverse complement of r2, or None: forward offsets
    0, 1, .. while off < len1 - 30 (s1[off + i] against s2[i]), then backward 0, -1, .. while off > -(len2 - 30)
    (s1[i] against s2[-off + i]); accepted iff the mismatches among the first min(50, ol) positions are at most
    min(5, ol * 20 // 100).  (Every offset of a direction is scored at once with numpy; the first accepted wins.)"""
    import numpy as np
    s2 = revcomp(r2)
    a = np.frombuffer(s1, dtype=np.uint8)
    b = np.frombuffer(s2, dtype=np.uint8)
    len1, len2, req = len(a), len(b), 30
    for direction in (1, -1):
        x, y = (a, b) if direction == 1 else (b, a)   # backward: s2 shifted against s1 is s1 against s2, mirrored
        nx, ny = len(x), len(y)
        noff = nx - req if direction == 1 else len2 - req
        if noff <= 0:
            continue
        offs = np.arange(noff)
        xp = np.concatenate([x, np.zeros(50, dtype=np.uint8)])
        yp = np.concatenate([y, np.zeros(50, dtype=np.uint8)])
        win = xp[offs[:, None] + np.arange(50)[None, :]]          # x[off + i]
        ol = np.minimum(nx - offs, ny)
        n = np.minimum(50, ol)
        diff = (win != yp[None, :50]) & (np.arange(50)[None, :] < n[:, None])
        ok = diff.sum(axis=1) <= np.minimum(5, ol * 20 // 100)
        hit = np.flatnonzero(ok)
        if hit.size:
            k = int(hit[0])
            return (k, int(ol[k])) if direction == 1 else (-k, int(ol[k]))
    return None


def _trim(rec, F, T):
    h, s, q = rec
    if F + T > len(s):
        return None
    s, q = s[F:len(s) - T], q[F:len(q) - T]
    n = poly_g(s)
    return h, s[:n], q[:n]


def clean_sample(r1, r2, singles, F=10, T=10, adapter=True, merge=True, dedup=True):
    """Clean one sample: r1 / r2 = its paired records (lists of equal length), singles = its single-end records.
    Returns (FASTQ text, stats) with stats = dict(clean_bp, records, base[40][4] (A C G T), reach[40])."""
    assert len(r1) == len(r2)
    out = []             # (header, seq, qual, counts_for_base_frequency)
    first_group = "pairs" if r1 else "singles"
    seen = set()
    for a, b in zip(r1, r2):
        if dedup:
            key = (a[1], b[1])
            if key in seen:
                continue
            seen.add(key)
        a, b = _trim(a, F, T), _trim(b, F, T)
        if a is None or b is None:
            continue
        (h1, s1, q1), (h2, s2, q2) = a, b
        if adapter:
            ov = overlap(s1, s2)
            if ov is not None and ov[0] < 0:
                s1, q1 = s1[:min(len(s1), ov[1] + F)], q1[:min(len(q1), ov[1] + F)]
                s2, q2 = s2[:min(len(s2), ov[1] + F)], q2[:min(len(q2), ov[1] + F)]
        ov = overlap(s1, s2) if merge else None
        if ov is not None:
            off, ol = ov
            n1 = ol + max(0, off)
            seq, qual = s1[:n1], q1[:n1]
            if off > 0:
                seq += revcomp(s2)[ol:]
                qual += q2[::-1][ol:]
            out.append((h1, seq, qual, first_group == "pairs"))
        else:
            out.append((h1, s1, q1, first_group == "pairs"))
            out.append((h2, s2, q2, False))
    seen = set()
    for rec in singles:
        if dedup:
            if rec[1] in seen:
                continue
            seen.add(rec[1])
        t = _trim(rec, F, T)
        if t is None:
            continue
        out.append(t + (first_group == "singles",))
    text = bytearray()
    base = [[0] * 4 for _ in range(CYCLES)]
    reach = [0] * CYCLES
    bp = nrec = 0
    for h, s, q, counted in out:
        if not s:
            continue
        text += h + b"\n" + s + b"\n+\n" + q + b"\n"
        bp += len(s)
        nrec += 1
        if counted:
            for c in range(min(CYCLES, len(s))):
                reach[c] += 1
                j = b"ACGT".find(s[c:c + 1])
                if j >= 0:
                    base[c][j] += 1
    return bytes(text), dict(clean_bp=bp, records=nrec, base=base, reach=reach)


# ------------------------------------------------------------------ cases ----

def fq(records):
    """FASTQ text of (header line, seq, qual) records."""
    return b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in records)


def _rng_seq(rng, n, alphabet=b"ACGT"):
    import numpy as np
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


def _qual(rng, n):
    import numpy as np
    return bytes((rng.integers(0, 41, n) + 33).astype(np.uint8))


def pair_from_insert(rng, name, insert, L, adapter1=b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA",
                     adapter2=b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"):
    """(R1, R2) records of a fragment: R1 reads the insert forward, R2 its reverse complement; a read longer than
    the insert runs into its adapter (then into poly-G, as a two-colour instrument does)."""
    pad = b"G" * L
    r1 = (insert + adapter1 + pad)[:L]
    r2 = (revcomp(insert) + adapter2 + pad)[:L]
    return ((b"@" + name + b" 1:N:0", r1, _qual(rng, L)), (b"@" + name + b" 2:N:0", r2, _qual(rng, L)))


def hand_cases():
    """{name: dict(r1, r2, singles, F, T)}: the boundaries of every rule (tests/test_clean_rules.py states what
    each must give; the GPU must give what clean_sample gives)."""
    import numpy as np
    rng = np.random.default_rng(11)
    cases = {}

    def se(name, seq):
        return (b"@" + name, seq, _qual(rng, len(seq)))

    A20, C20 = b"A" * 20, b"C" * 20
    tail5 = bytearray(b"G" * 60)
    for i in (7, 15, 23, 31, 39):
        tail5[59 - i] = ord("A")
    tail6 = bytearray(tail5)
    tail6[59 - 47] = ord("A")
    early = bytearray(b"G" * 20)
    for i in (7, 8):
        early[19 - i] = ord("A")
    every8 = bytearray(b"G" * 40)
    for i in (7, 15, 23, 31):
        every8[39 - i] = ord("A")
    cases["poly_g"] = dict(r1=[], r2=[], F=0, T=0, singles=[
        se(b"g7", A20 + b"G" * 7), se(b"g8", A20 + b"G" * 8), se(b"g9", A20 + b"G" * 9), se(b"g10", A20 + b"G" * 10),
        se(b"every8", C20 + bytes(every8)), se(b"two_early", C20 + bytes(early)), se(b"mism5", C20 + bytes(tail5)),
        se(b"mism6", C20 + bytes(tail6)), se(b"allG", b"G" * 30), se(b"empty", b""), se(b"short", b"GGG")])
    L = 100
    ins = {n: _rng_seq(rng, n) for n in (169, 170, 200, 100, 60)}
    r1, r2 = [], []
    for n, seqs in ins.items():
        a, b = pair_from_insert(rng, b"ins%d" % n, seqs, L)
        r1.append(a)
        r2.append(b)
    cases["overlap_lengths"] = dict(r1=r1, r2=r2, singles=[], F=0, T=0)
    # mismatches in the first 50 compared positions (limit 5) and past them
    base = _rng_seq(rng, 200)
    r1, r2 = [], []
    for tag, where in ((b"m5", (1, 9, 17, 25, 33)), (b"m6", (1, 9, 17, 25, 33, 41)), (b"late10", tuple(range(60, 70)))):
        a, b = pair_from_insert(rng, tag, base, 150)
        s2 = bytearray(b[1])
        for i in where:    # s2 = rc(R2); overlap position i of s2 is R2[len - 1 - i]
            s2[149 - i] = ord("A") if s2[149 - i] != ord("A") else ord("C")
        r1.append(a)
        r2.append((b[0], bytes(s2), b[2]))
    cases["mismatch_limit"] = dict(r1=r1, r2=r2, singles=[], F=0, T=0)
    # read-through into the adapter, with and without front trim
    short = _rng_seq(rng, 120)
    a, b = pair_from_insert(rng, b"rt", short, 150)
    cases["readthrough_F0"] = dict(r1=[a], r2=[b], singles=[], F=0, T=0)
    cases["readthrough_F10"] = dict(r1=[a], r2=[b], singles=[], F=10, T=10)
    cases["readthrough_F7_T3"] = dict(r1=[a], r2=[b], singles=[], F=7, T=3)
    # F + T against the length
    cases["trim_bounds"] = dict(F=10, T=10, singles=[se(b"l19", _rng_seq(rng, 19)), se(b"l20", _rng_seq(rng, 20)),
                                                     se(b"l21", _rng_seq(rng, 21))],
                                r1=[se(b"p19", _rng_seq(rng, 19)), se(b"p20", _rng_seq(rng, 20)), se(b"p60", _rng_seq(rng, 60))],
                                r2=[se(b"p19", _rng_seq(rng, 80)), se(b"p20", _rng_seq(rng, 80)), se(b"p60", _rng_seq(rng, 20))])
    # duplicates: SE by sequence, PE by both mates; qualities and names differ
    s1, s2, s3 = _rng_seq(rng, 80), _rng_seq(rng, 80), _rng_seq(rng, 80)
    cases["duplicates"] = dict(F=0, T=0, singles=[se(b"a", s1), se(b"b", s2), se(b"a_again", s1), se(b"c", s1 + b"A")],
                               r1=[se(b"x", s1), se(b"y", s1), se(b"x_again", s1), se(b"z", s2)],
                               r2=[se(b"x", s2), se(b"y", s3), se(b"x_again", s2), se(b"z", s2)])
    # bytes that are not ACGT: N in both mates (equal), lower case (compared as bytes)
    ins = _rng_seq(rng, 170)
    a, b = pair_from_insert(rng, b"nn", ins, 100)
    a1, b1 = bytearray(a[1]), bytearray(b[1])
    a1[80], b1[100 - 1 - (170 - 1 - 80)] = ord("N"), ord("N")
    a1[90] = ord("a")
    cases["non_acgt"] = dict(r1=[(a[0], bytes(a1), a[2])], r2=[(b[0], bytes(b1), b[2])], singles=[se(b"n", b"NNNNACGTNNNN" * 5)],
                             F=0, T=0)
    return cases


def synth_set(seed, npairs, nsingles, L=150, dup_frac=0.1):
    """Seeded raw reads: fragments shorter than, equal to and longer than the reads (adapters, then poly-G, where a
    read runs past its fragment), N bases, ~dup_frac exact duplicates; (r1, r2, singles)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    r1, r2, singles = [], [], []
    for p in range(npairs):
        if p and rng.random() < dup_frac:
            j = int(rng.integers(0, p))
            r1.append((b"@dup%d" % p, r1[j][1], r1[j][2]))
            r2.append((b"@dup%d" % p, r2[j][1], r2[j][2]))
            continue
        kind = rng.random()
        n = int(rng.integers(40, L)) if kind < 0.3 else (L if kind < 0.35 else int(rng.integers(L + 1, 2 * L + 100)))
        ins = bytearray(_rng_seq(rng, n))
        for i in np.flatnonzero(rng.random(n) < 0.003):
            ins[i] = ord("N")
        a, b = pair_from_insert(rng, b"p%d" % p, bytes(ins), L)
        r1.append(a)
        r2.append(b)
    for q in range(nsingles):
        if q and rng.random() < dup_frac:
            j = int(rng.integers(0, q))
            singles.append((b"@sdup%d" % q, singles[j][1], singles[j][2]))
            continue
        n = int(rng.integers(20, L + 1))
        s = _rng_seq(rng, n) + (b"G" * int(rng.integers(0, 30)) if rng.random() < 0.2 else b"")
        singles.append((b"@s%d" % q, s, _qual(rng, len(s))))
    return r1, r2, singles
