"""Named cases of the read screen (`--exclude-fasta` / `--keep-fasta`), each a few hundred bytes: a reference FASTA, K,
min_hits and one or more samples of cleaned FASTQ text.  `expect`, where given, says per sample and record whether the
read matches -- what the case is FOR; tests/test_screen_rules.py holds tests/screen_ref.py to it, the emulation and the
GPU tests hold the device code to screen_ref.  TILE is the small tile the tile cases are built around (VKIMG_SCREEN_TILE)."""
import random
from collections import namedtuple

Case = namedtuple("Case", "name fasta k min_hits samples expect")

TILE = 64
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def fq(reads, eol=b"\n", last_eol=True, names=None):
    """Cleaned FASTQ text of the reads, four lines each."""
    out = bytearray()
    for i, r in enumerate(reads):
        name = names[i] if names else b"r%d" % i
        out += b"@" + name + eol + r + eol + b"+" + eol + b"I" * len(r) + eol
    if not last_eol and out:
        out = out[:len(out) - len(eol)]
    return bytes(out)


def fa(records, width=60, eol=b"\n"):
    """FASTA text: (name, sequence) records wrapped at `width`."""
    out = bytearray()
    for name, s in records:
        out += b">" + name + eol
        for i in range(0, len(s), width):
            out += s[i:i + width] + eol
    return bytes(out)


def _read_cases():
    rng = random.Random(20240611)
    out = []
    K = 21
    # lengths K - 1, K, K + 1 of a read cut from the reference
    ref = seq(rng, 60)
    out.append(Case("len_k_minus_1_k_k_plus_1", fa([(b"ref", ref)]), K, 1, [fq([ref[:K - 1], ref[:K], ref[:K + 1]])],
                    [[False, True, True]]))
    # reads of 63, 64, 65, 128, 129 windows: the only matching window the first, the last, none
    for nwin in (63, 64, 65, 128, 129):
        r = seq(rng, nwin + K - 1)
        other = seq(rng, nwin + K - 1)
        out.append(Case("windows_%d_first" % nwin, fa([(b"w", r[:K])]), K, 1, [fq([other, r])], [[False, True]]))
        out.append(Case("windows_%d_last" % nwin, fa([(b"w", rc(r[-K:]))]), K, 1, [fq([r, other])], [[True, False]]))
    # one read of 3 tiles plus a few bases (tiles of TILE bases overlap by K - 1): the only matching window the first, the
    # last, the last of a tile, the first of the next, one that lies across a tile's last base
    step = TILE - (K - 1)
    L = 3 * step + (K - 1) + 5
    r = seq(rng, L)
    spots = [0, L - K]
    for t in (1, 2, 3):
        spots += [t * step - 1, t * step, t * step + 6, (t - 1) * step + TILE - K // 2]
    for p in sorted(set(p for p in spots if 0 <= p <= L - K)):
        out.append(Case("tiles_window_at_%d" % p, fa([(b"w", r[p:p + K])]), K, 1, [fq([r])], [[True]]))
    # a match only as reverse complement; lower case against upper case and the converse
    r = seq(rng, 80)
    out.append(Case("revcomp_only", fa([(b"w", rc(r[30:30 + K]))]), K, 1, [fq([r])], [[True]]))
    out.append(Case("lower_read_upper_ref", fa([(b"w", r[10:10 + K])]), K, 1, [fq([r.lower()])], [[True]]))
    out.append(Case("upper_read_lower_ref", fa([(b"w", r[10:10 + K].lower())]), K, 1, [fq([r])], [[True]]))
    out.append(Case("mixed_case", fa([(b"w", r[10:10 + K].swapcase()[:7] + r[17:10 + K])]), K, 1,
                    [fq([r[:20].lower() + r[20:]])], [[True]]))
    # N inside the only matching window (no match) and next to it (match)
    w0 = 30
    inside = r[:w0 + 9] + b"N" + r[w0 + 10:]
    before = r[:w0 - 1] + b"N" + r[w0:]
    after = r[:w0 + K] + b"N" + r[w0 + K + 1:]
    out.append(Case("n_in_and_beside_the_window", fa([(b"w", r[w0:w0 + K])]), K, 1, [fq([inside, before, after])],
                    [[False, True, True]]))
    # min_hits 1, 2, 3 with exactly n - 1 and n hit positions: one key at several positions (positions are counted, not
    # distinct keys), and distinct keys; an N behind every copy keeps the neighbouring windows out
    x, y, z = seq(rng, K), seq(rng, K), seq(rng, K)
    for n in (1, 2, 3):
        fewer = seq(rng, 9) + b"N".join([x] * (n - 1) + [seq(rng, 12)])
        enough = seq(rng, 9) + b"N".join([x] * n + [seq(rng, 12)])
        out.append(Case("min_hits_%d_one_key" % n, fa([(b"x", x)]), K, n, [fq([fewer, enough])], [[False, True]]))
        keys = [x, rc(y), z]
        fewer = b"N".join(keys[:n - 1] + [seq(rng, 15)])
        enough = b"N".join(keys[:n] + [seq(rng, 15)])
        out.append(Case("min_hits_%d_distinct_keys" % n, fa([(b"x", x), (b"y", y), (b"z", z)]), K, n, [fq([fewer, enough])],
                        [[False, True]]))
    # adjacent positions: a read cut from the reference with L - K + 1 hits
    ref = seq(rng, 100)
    out.append(Case("min_hits_3_adjacent", fa([(b"ref", ref)]), K, 3, [fq([ref[5:5 + K + 1], ref[40:40 + K + 2]])],
                    [[False, True]]))
    # a palindromic key (its own reverse complement) at K = 16 and 30
    for k in (16, 30):
        half = seq(rng, k // 2)
        pal = half + rc(half)
        out.append(Case("palindrome_k%d" % k, fa([(b"p", pal)]), k, 1, [fq([seq(rng, 11) + pal + seq(rng, 7), seq(rng, 50)])],
                        [[True, False]]))
    # K = 16, 21, 31: reads cut from either strand of a wrapped reference, and reads from elsewhere
    ref = seq(rng, 200)
    for k in (16, 21, 31):
        reads = [ref[20:90], rc(ref[100:170]), seq(rng, 70), ref[150:150 + k], rc(ref[3:3 + k - 1])]
        out.append(Case("either_strand_k%d" % k, fa([(b"ref", ref)]), k, 1, [fq(reads)], [[True, True, False, True, False]]))
    # \r\n records, a last record without \n, both
    reads = [ref[20:70], seq(rng, 50), rc(ref[120:170]), seq(rng, 40)]
    want = [[True, False, True, False]]
    out.append(Case("crlf_records", fa([(b"ref", ref)]), K, 1, [fq(reads, eol=b"\r\n")], want))
    out.append(Case("no_last_newline", fa([(b"ref", ref)]), K, 1, [fq(reads, last_eol=False)], want))
    out.append(Case("no_last_newline_last_kept", fa([(b"ref", ref)]), K, 1, [fq(reads[:3], last_eol=False)], [want[0][:3]]))
    out.append(Case("crlf_no_last_newline", fa([(b"ref", ref)]), K, 1, [fq(reads[:3], eol=b"\r\n", last_eol=False)], [want[0][:3]]))
    # a sample of zero records; one in which every record matches and one in which none does; an empty read
    hit = [ref[i:i + 60] for i in (0, 30, 77, 140)]
    miss = [seq(rng, 60) for _ in range(4)]
    out.append(Case("zero_records", fa([(b"ref", ref)]), K, 1, [b""], [[]]))
    out.append(Case("all_and_none", fa([(b"ref", ref)]), K, 1, [fq(hit), fq(miss)], [[True] * 4, [False] * 4]))
    out.append(Case("empty_read", fa([(b"ref", ref)]), K, 1, [fq([b"", ref[:40], b""])], [[False, True, False]]))
    # three samples in one call, an empty one among them; under either mode the first kept record of a sample is not
    # always its first
    s0 = fq([miss[0], hit[0], hit[1], miss[1]], names=[b"a0", b"a1", b"a2", b"a3"])
    s1 = fq([hit[2], miss[2], hit[3]], eol=b"\r\n", names=[b"b0", b"b1", b"b2"])
    s2 = fq([hit[0], hit[3], miss[3], miss[0], hit[1]], last_eol=False)
    out.append(Case("three_samples", fa([(b"ref", ref)]), K, 1, [s0, s1, s2],
                    [[False, True, True, False], [True, False, True], [True, True, False, False, True]]))
    out.append(Case("three_samples_one_empty", fa([(b"ref", ref)]), K, 1, [s0, b"", s2],
                    [[False, True, True, False], [], [True, True, False, False, True]]))
    # the empty set: a reference of records shorter than K
    out.append(Case("empty_set", fa([(b"a", ref[:K - 1]), (b"b", ref[50:50 + 5])]), K, 1, [s0, s1, s2],
                    [[False] * 4, [False] * 3, [False] * 5]))
    return out


def _reference_cases():
    """Cases about the reference's text; the sample probes what must and must not be in the set."""
    rng = random.Random(7)
    out = []
    ref = seq(rng, 150)
    probe = [ref[:60], rc(ref[80:150]), seq(rng, 60)]
    want = [[True, True, False]]
    for k in (21, 31):
        out.append(Case("ref_width_60_k%d" % k, fa([(b"r", ref)], 60), k, 1, [fq(probe)], want))
        out.append(Case("ref_width_7_k%d" % k, fa([(b"r", ref)], 7), k, 1, [fq(probe)], want))   # (K = 31: a window over five lines)
    out.append(Case("ref_unwrapped", fa([(b"r", ref)], 1000), 21, 1, [fq(probe)], want))
    out.append(Case("ref_crlf", fa([(b"r", ref)], 13, eol=b"\r\n"), 21, 1, [fq(probe)], want))
    out.append(Case("ref_no_last_newline", fa([(b"r", ref)], 60)[:-1], 21, 1, [fq(probe)], want))
    out.append(Case("ref_ends_in_cr", fa([(b"r", ref)], 60, eol=b"\r\n")[:-1], 21, 1, [fq(probe)], want))
    blank = fa([(b"r", ref)], 25).replace(b"\n", b"\n\n", 3)
    out.append(Case("ref_blank_lines", blank, 21, 1, [fq(probe)], want))
    # a \r inside a line is a byte like any other non-base: the windows across it do not exist
    K = 21
    inner = b">r\n" + ref[:40] + b"\r" + ref[40:80] + b"\n"
    out.append(Case("ref_cr_inside_a_line", inner, K, 1, [fq([ref[25:55], ref[:40], ref[45:80]])], [[False, True, True]]))
    # N runs: the windows across them do not exist
    nrun = ref[:50] + b"NNNN" + ref[50:100] + b"n" + ref[100:]
    out.append(Case("ref_n_runs", fa([(b"r", nrun)], 60), K, 1, [fq([ref[35:65], ref[85:115], ref[:50], ref[101:150]])],
                    [[False, False, True, True]]))
    # other non-bases (IUPAC codes, a digit, a gap)
    iupac = ref[:30] + b"R" + ref[30:60] + b"-" + ref[60:90] + b"5" + ref[90:]
    out.append(Case("ref_other_bytes", fa([(b"r", iupac)], 60), K, 1, [fq([ref[15:45], ref[:30], ref[91:150], ref[45:75]])],
                    [[False, True, True, False]]))
    # two records whose junction would form a key that must not exist; a header-only record between two others
    a, b = ref[:70], ref[70:]
    out.append(Case("ref_junction", fa([(b"a", a), (b"b", b)], 60), K, 1, [fq([ref[55:85], a[-30:], b[:30]])], [[False, True, True]]))
    out.append(Case("ref_header_only_record", fa([(b"a", a), (b"none", b""), (b"b", b)], 60), K, 1,
                    [fq([ref[55:85], a[-30:], b[:30]])], [[False, True, True]]))
    out.append(Case("ref_header_only", b">nothing here\n", K, 1, [fq(probe)], [[False] * 3]))
    out.append(Case("ref_empty_text", b"", K, 1, [fq(probe)], [[False] * 3]))
    # only records shorter than K: the empty set
    out.append(Case("ref_short_records", fa([(b"a", ref[:K - 1]), (b"b", ref[30:40]), (b"c", b"")], 7), K, 1, [fq(probe)],
                    [[False] * 3]))
    # one sequence repeated 100 times, as records and on one line with a break between the copies: the distinct count is one copy's
    unit = ref[:40]
    out.append(Case("ref_repeat_100_records", fa([(b"u%d" % i, unit) for i in range(100)], 60), K, 1, [fq([unit, ref[60:100]])],
                    [[True, False]]))
    out.append(Case("ref_repeat_100_line", fa([(b"u", b"N".join([unit] * 100))], 61), K, 1, [fq([unit, ref[60:100]])],
                    [[True, False]]))
    # 1,000 windows, every key distinct: the table at its minimum size for them (and, forced, at 1,024 slots)
    big = seq(rng, 1000 + K - 1)
    out.append(Case("ref_1000_keys", fa([(b"big", big)], 70), K, 1, [fq([big[500:560], rc(big[:30]), seq(rng, 60)])],
                    [[True, True, False]]))
    return out


READ_CASES = _read_cases()
REFERENCE_CASES = _reference_cases()
ALL_CASES = READ_CASES + REFERENCE_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
