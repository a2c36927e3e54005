"""Adapter detection and trimming by sequence in step B (`image --from-raw --detect-adapters / --adapter-sequence`)
restated in Python: the contract that vk_clean_detect_device and vk_clean_adapters_device meet byte for byte
("Step B").  detect_adapter and trim_by_sequence are vectorised with numpy over windows, occurrences
and offsets; trim_by_sequence_literal is the rule one comparison at a time, and the tests hold the two equal.
clean_sample_adapters is clean_ref.clean_sample with the new step in its place.  Plus the seeded read sets that the
CPU and GPU tests share.  Tests only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_ref as R  # noqa: E402

from varkoder_amd.adapters import snap  # noqa: E402

EVAL_RECORDS = 262144     # records of a group that detection reads
SEED_K = 10               # seed length
SEED_FROM = 20            # first read position of a counted window
TOP = 10                  # candidates ranked
FOLD = 20                 # a candidate's count * 4^10 // total must exceed this
MIN_VOTES = 50            # fewer live occurrences than this: the extension ran out
CONSENSUS_PCT = 95        # the top byte needs this share of the votes
MAX_DETECTED = 60         # bases of a detected string kept

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _b in enumerate(b"ACGT"):
    _CODE[_b] = _i


def _matrix(reads):
    """reads as a zero-padded byte matrix [n, max len + 1] and their lengths."""
    n = len(reads)
    L = max((len(s) for s in reads), default=0) + 1
    m = np.zeros((n, L), dtype=np.uint8)
    for i, s in enumerate(reads):
        m[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return m, np.array([len(s) for s in reads], dtype=np.int64)


def _windows(m):
    """(keys, valid) of every 10-mer window start p of the matrix: key = the 2-bit codes A0 C1 G2 T3, first base most
    significant (so key order is lexicographic order); valid: the 10 bytes are ACGT (the zero padding never is)."""
    codes = _CODE[m]
    W = m.shape[1] - SEED_K + 1
    if W <= 0:
        return np.zeros((m.shape[0], 0), dtype=np.int64), np.zeros((m.shape[0], 0), dtype=bool)
    key = np.zeros((m.shape[0], W), dtype=np.int64)
    valid = np.ones((m.shape[0], W), dtype=bool)
    for i in range(SEED_K):
        c = codes[:, i:i + W]
        valid &= c != 255
        key = (key << 2) | (c & 3)
    return key, valid


def key_ok():
    """bool[4^10]: the keys that survive the filters (not A*10, no base 6 or more times, G + C under 8, no GGGG head)."""
    K = np.arange(4 ** SEED_K, dtype=np.int64)
    digits = np.stack([(K >> (2 * (SEED_K - 1 - i))) & 3 for i in range(SEED_K)])
    per = np.stack([(digits == b).sum(axis=0) for b in range(4)])
    ok = (K != 0) & (per.max(axis=0) < 6) & (per[1] + per[2] < 8) & ((K >> 12) != 0xAA)
    return ok


_KEY_OK = None


def key_str(key):
    return bytes(b"ACGT"[(key >> (2 * (SEED_K - 1 - i))) & 3] for i in range(SEED_K))


def candidates(reads):
    """[(key, count)] of the ranked keys that pass the fold threshold, and `total`."""
    global _KEY_OK
    if _KEY_OK is None:
        _KEY_OK = key_ok()
    m, _ = _matrix(reads)
    key, valid = _windows(m)
    valid[:, :SEED_FROM] = False
    counts = np.bincount(key[valid], minlength=4 ** SEED_K)
    counts[~_KEY_OK] = 0
    total = int(counts.sum())
    nz = np.flatnonzero(counts)
    order = nz[np.lexsort((nz, -counts[nz]))][:TOP]
    return [(int(k), int(counts[k])) for k in order if total and int(counts[k]) * 4 ** SEED_K // total > FOLD], total


def _extend(m, lens, occ_r, occ_p, forward, shift_tail):
    """(bytes chosen, ran out) of one direction of the extension of a seed's occurrences."""
    avail = (lens[occ_r] - shift_tail - (occ_p + SEED_K)) if forward else occ_p
    live = np.ones(len(occ_r), dtype=bool)
    out = bytearray()
    for j in range(int(avail.max(initial=0)) + 1):
        has = live & (avail > j)
        n = int(has.sum())
        if n < MIN_VOTES:
            return bytes(out), True
        col = occ_p + SEED_K + j if forward else occ_p - 1 - j
        b = m[occ_r, np.clip(col, 0, m.shape[1] - 1)]
        hist = np.bincount(b[has], minlength=256)
        top = int(np.argmax(hist))
        if int(hist[top]) * 100 < CONSENSUS_PCT * n:
            return bytes(out), False
        out.append(top)
        live = has & (b == top)
    return bytes(out), True


def extend(reads, key, T):
    """(D, backward ran out, forward ran out) of the seed `key` in `reads` (-T's tail value T); None when the seed has
    fewer than MIN_VOTES occurrences in the extension's range (both directions would run out at once: no evidence)."""
    m, lens = _matrix(reads)
    keys, valid = _windows(m)
    shift_tail = max(1, T)
    p = np.arange(keys.shape[1])[None, :]
    hit = valid & (keys == key) & (p >= SEED_FROM) & (p <= lens[:, None] - SEED_K - shift_tail)
    occ_r, occ_p = np.nonzero(hit)
    if len(occ_r) < MIN_VOTES:
        return None
    back, back_out = _extend(m, lens, occ_r, occ_p, False, shift_tail)
    fwd, fwd_out = _extend(m, lens, occ_r, occ_p, True, shift_tail)
    return (back[::-1] + key_str(key) + fwd)[:MAX_DETECTED], back_out, fwd_out


def detect_adapter(reads, T=10):
    """The adapter detected in a group's evaluation set (sequences, in file order; the first EVAL_RECORDS are read),
    or None."""
    reads = list(reads[:EVAL_RECORDS])
    cands, _ = candidates(reads)
    for key, _ in cands:
        ext = extend(reads, key, T)
        if ext is None:
            continue
        D, back_out, fwd_out = ext
        s = snap(D)
        if s is not None:
            return s
        if back_out and fwd_out:
            return D
    return None


def trim_start(alen):
    return -4 if alen >= 16 else -3 if alen >= 12 else -2 if alen >= 8 else 0


def trim_by_sequence_literal(seq, adapter):
    """fastp's trimBySequence, one comparison at a time: the read's new length."""
    rlen, alen = len(seq), len(adapter)
    pos = trim_start(alen)
    while pos < rlen - 4:
        cmplen = min(rlen - pos, alen)
        mism = sum(1 for i in range(max(0, -pos), cmplen) if adapter[i] != seq[i + pos])
        if mism <= cmplen // 8:
            return max(pos, 0)
        pos += 1
    return rlen


def trim_by_sequence(seq, adapter):
    """trim_by_sequence_literal with every offset scored at once."""
    rlen, alen = len(seq), len(adapter)
    start = trim_start(alen)
    if start >= rlen - 4:
        return rlen
    pos = np.arange(start, rlen - 4)
    i = np.arange(alen)[None, :]
    cmplen = np.minimum(rlen - pos, alen)
    idx = pos[:, None] + i
    counted = (idx >= 0) & (i < cmplen[:, None])
    s = np.frombuffer(seq, dtype=np.uint8)
    a = np.frombuffer(adapter, dtype=np.uint8)
    diff = (s[np.clip(idx, 0, rlen - 1)] != a[None, :]) & counted
    ok = np.flatnonzero(diff.sum(axis=1) <= cmplen // 8)
    return max(int(pos[ok[0]]), 0) if ok.size else rlen


def group_adapters(r1, r2, singles, T=10, detect=True, explicit=None, explicit_r2=None):
    """[R1's, R2's, the single reads'] adapter (bytes or None) of one sample: explicit sequences win for their groups,
    detection (with `detect`) fills the others."""
    a2 = explicit_r2 if explicit_r2 is not None else explicit
    out = []
    for recs, given in ((r1, explicit), (r2, a2), (singles, explicit)):
        if given is not None:
            out.append(given)
        elif detect and recs:
            out.append(detect_adapter([s for _, s, _ in recs[:EVAL_RECORDS]], T))
        else:
            out.append(None)
    return out


def clean_sample_adapters(r1, r2, singles, F=10, T=10, adapter=True, merge=True, dedup=True, adapters=(None, None, None)):
    """clean_ref.clean_sample with trimming by sequence: adapters = [R1's, R2's, the single reads'] (bytes or None).
    Single reads are trimmed after poly-G; a pair's mates are trimmed (R2 as read) when the overlap did not cut the
    pair, before the merge.  Returns (FASTQ text, stats, dict(reads, bases) trimmed by sequence)."""
    assert len(r1) == len(r2)
    a1, a2, ase = adapters if adapter else (None, None, None)
    ad = dict(reads=0, bases=0)

    def cut(s, q, a):
        if a is None:
            return s, q
        n = trim_by_sequence(s, a)
        if n < len(s):
            ad["reads"] += 1
            ad["bases"] += len(s) - n
        return s[:n], q[:n]

    out = []
    first_group = "pairs" if r1 else "singles"
    seen = set()
    for a, b in zip(r1, r2):
        if dedup:
            key = (a[1], b[1])
            if key in seen:
                continue
            seen.add(key)
        a, b = R._trim(a, F, T), R._trim(b, F, T)
        if a is None or b is None:
            continue
        (h1, s1, q1), (h2, s2, q2) = a, b
        if adapter:
            ov = R.overlap(s1, s2)
            if ov is not None and ov[0] < 0:
                s1, q1 = s1[:min(len(s1), ov[1] + F)], q1[:min(len(q1), ov[1] + F)]
                s2, q2 = s2[:min(len(s2), ov[1] + F)], q2[:min(len(q2), ov[1] + F)]
            else:
                s1, q1 = cut(s1, q1, a1)
                s2, q2 = cut(s2, q2, a2)
        ov = R.overlap(s1, s2) if merge else None
        if ov is not None:
            off, ol = ov
            n1 = ol + max(0, off)
            seq, qual = s1[:n1], q1[:n1]
            if off > 0:
                seq += R.revcomp(s2)[ol:]
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
        t = R._trim(rec, F, T)
        if t is None:
            continue
        h, s, q = t
        s, q = cut(s, q, ase)
        out.append((h, s, q, first_group == "singles"))
    text = bytearray()
    base = [[0] * 4 for _ in range(R.CYCLES)]
    reach = [0] * R.CYCLES
    bp = nrec = 0
    for h, s, q, counted in out:
        if not s:
            continue
        text += h + b"\n" + s + b"\n+\n" + q + b"\n"
        bp += len(s)
        nrec += 1
        if counted:
            for c in range(min(R.CYCLES, len(s))):
                reach[c] += 1
                j = b"ACGT".find(s[c:c + 1])
                if j >= 0:
                    base[c][j] += 1
    return bytes(text), dict(clean_bp=bp, records=nrec, base=base, reach=reach), ad


# ------------------------------------------------------------------ cases ----

TRUSEQ1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
TRUSEQ2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
NEXTERA = b"CTGTCTCTTATACACATCT"
UNLISTED = b"GTCAGTTACCGATGCATTGCACGTTAGCCTAGT"   # in no table: random bases


def _rng_seq(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def _qual(rng, n):
    return bytes((rng.integers(0, 41, n) + 33).astype(np.uint8))


def se_readthrough(seed, n, frac, adapter=TRUSEQ1, L=150, insert=(30, 140), tail=b"G"):
    """n single reads of L bases: a fraction `frac` read an insert of a random length in [insert) and run into
    `adapter`, then into `tail` repeated; the rest are genome.  Records (header, seq, qual)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if rng.random() < frac:
            k = int(rng.integers(*insert))
            s = (_rng_seq(rng, k) + adapter + tail * L)[:L]
        else:
            s = _rng_seq(rng, L)
        out.append((b"@r%d" % i, s, _qual(rng, L)))
    return out


def dimers(seed, n, frac, seq=UNLISTED, L=100):
    """A fraction of reads that are all `seq` over and over from position 0 (adapter dimers, no insert)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = (seq * (L // len(seq) + 1))[:L] if rng.random() < frac else _rng_seq(rng, L)
        out.append((b"@d%d" % i, s, _qual(rng, L)))
    return out


def repeat_reads(seed, n, frac, L=150):
    """A genomic repeat: a fraction of reads hold a 40-base element at a random place, in random sequence (the
    consensus breaks on both sides of it)."""
    rng = np.random.default_rng(seed)
    unit = _rng_seq(np.random.default_rng(999), 40)
    out = []
    for i in range(n):
        s = bytearray(_rng_seq(rng, L))
        if rng.random() < frac:
            at = int(rng.integers(25, L - 45))
            s[at:at + 40] = unit
        out.append((b"@g%d" % i, bytes(s), _qual(rng, L)))
    return out


def pairs_with_adapters(seed, n, short_frac, adapter1=TRUSEQ1, adapter2=TRUSEQ2, L=150, short=(8, 30)):
    """n pairs: a fraction have inserts of `short` bases (under the overlap's 30, so the overlap cannot see them),
    the rest long inserts (some read through: overlap-trimmed); R1 into adapter1, R2 into adapter2."""
    rng = np.random.default_rng(seed)
    r1, r2 = [], []
    for i in range(n):
        k = int(rng.integers(*short)) if rng.random() < short_frac else int(rng.integers(60, 2 * L))
        a, b = R.pair_from_insert(rng, b"q%d" % i, _rng_seq(rng, k), L, adapter1, adapter2)
        r1.append(a)
        r2.append(b)
    return r1, r2
