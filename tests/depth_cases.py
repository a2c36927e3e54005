"""Inputs for the depth filter (tests/depth_ref.py is the rule): the smallest at which the kernel can go wrong, each at
K = 16, 21 and 31.  A case is its samples, K, the values of `every` to run it with, its band sets -- every set one
(lo, hi) per sample, a call each -- and the forced table size (None: the engine's).  Built once at import, deterministic."""
import random
from collections import namedtuple

import screen_ref
import spectrum_cases as SC
from screen_cases import fq, rc, seq
from spectrum_cases import distinct_kmers

Case = namedtuple("Case", "name samples k everys bandsets slots")

TILE = SC.TILE   # VKIMG_SPECTRUM_TILE of the small-tile runs
KS = SC.KS
OPEN = 2 ** 32 - 1


def copies(s, m):
    """m reads of s, a third of them its reverse complement."""
    return [s if i % 3 else rc(s) for i in range(m)]


def _cases(k):
    rng = random.Random(2000 + k)
    out = []

    def add(name, samples, bandsets, everys=(1,), slots=None):
        samples = [bytes(s) for s in samples]
        sets = [[b] * len(samples) if isinstance(b, tuple) else list(b) for b in bandsets]
        assert all(len(s) == len(samples) for s in sets)
        out.append(Case("%s_k%d" % (name, k), samples, k, tuple(everys), sets, slots))

    # n = 0, 1, 2, 3, 4 taken windows: the four k-mers of one read of K + 3 bases come 4, 6, 3 and 6 times, so the read
    # of two windows has depths 4 and 6 and the lower one decides
    base = seq(rng, k + 3)
    reads = [base[:k - 1], base[:k], base[:k + 1], base[:k + 2], base, b"N" * (k + 5), b""]
    for i, m in enumerate((0, 3, 1, 5)):
        reads += copies(base[i:i + k], m)
    add("n_0_to_4", [fq(reads)], [(0, OPEN), (1, OPEN), (0, 0), (5, OPEN), (0, 4), (4, 4), (6, 6)])

    # the median at the band's edges: windows of depth 5 and of depth 1, 3 and 2, 2 and 3, 2 and 2, an N between the halves
    reads = []
    for na, nb in ((3, 2), (2, 3), (2, 2)):
        a, b = seq(rng, k + na - 1), seq(rng, k + nb - 1)
        reads += [a + b"N" + b] + copies(a, 4)
    add("median_at_the_edges", [fq(reads)],
        [(lo, OPEN) for lo in (1, 2, 5, 6)] + [(0, hi) for hi in (1, 2, 5, 6)] + [(2, 5), (1, 1), (5, 5), (2, 4)])

    # above the histogram: single-window reads of multiplicity 254 .. 300; the decisions stay exact
    mers = distinct_kmers(rng, 5, k)
    reads = []
    for s, m in zip(mers, (254, 255, 256, 257, 300)):
        reads += copies(s, m)
    rng.shuffle(reads)
    add("above_the_histogram", [fq(reads)],
        [(lo, OPEN) for lo in (255, 256, 257, 300, 301)] + [(0, hi) for hi in (254, 255, 256, 299, 300)] + [(256, 257), (301, OPEN - 1)])

    # a read of 3 TILE + 17 bases with an N K bases before its end: an even number n of windows, all before the N, half of
    # them at depth 3 and half at depth 1 -- so one window lost turns the median from 1 to 3 where the lost one had depth
    # 1, and one window counted twice does where it had depth 3.  The K - 1 windows across the first seam (they start at
    # TILE - K + 1 .. TILE - 1) have depth 1 in the first read and depth 3 in the second.
    reads = []
    for seam_deep in (False, True):
        long_read = bytearray(seq(rng, 3 * TILE + 17))
        long_read[len(long_read) - k] = ord("N")
        long_read = bytes(long_read)
        n = len(long_read) - 2 * k + 1
        assert n % 2 == 0 and n // 2 > TILE
        first = 0 if seam_deep else n // 2   # the first of the n / 2 windows of depth 3
        reads += [long_read] + copies(long_read[first:first + n // 2 + k - 1], 2)
    add("tile_seam", [fq(reads)], [(0, 1), (2, OPEN), (0, OPEN), (3, 3)])

    # all lanes on one bin: more than 64 and more than 256 windows of one or two keys, an ordinary read behind each
    add("all_lanes_on_one_bin", [fq([b"A" * 600, seq(rng, 70), b"ACGT" * 150, seq(rng, 90), b"A" * 100])],
        [(0, OPEN), (2, OPEN), (0, 1), (586, 686), (0, 600)])

    # kept records are copied byte for byte
    a, b = seq(rng, 75), seq(rng, 60)
    rows = [a, rc(a), b.lower(), rc(b), seq(rng, 50)]
    add("byte_for_byte", [fq(rows, eol=b"\r\n"), fq(rows, last_eol=False), fq(rows[::-1], eol=b"\r\n", last_eol=False)],
        [(2, OPEN), (0, 1), (0, OPEN)])

    # every = 1, 2, 16: windows that are not taken do not count; a read without a taken window has depth 0
    sample = SC.BY_NAME["random_every_k%d" % k].samples[0]
    seqs = [s for _, s in screen_ref.split_records(sample)[1]]
    add("random_every", [fq(seqs + [s[:k + 2] for s in seqs[:40]])], [(2, OPEN), (0, 1), (1, 3), (0, 0)], everys=(1, 2, 16))

    # several samples in one call, a band each: an empty sample, bad framing between good samples
    good = fq([seq(rng, 100), seq(rng, 90)] + copies(seq(rng, 64), 3))
    add("several_samples", [good, b"", good, good[1:], good, good.replace(b"\n+\n", b"\n-\n", 1), good],
        [[(0, OPEN), (1, 2), (0, 1), (0, OPEN), (3, OPEN), (0, 0), (2, 3)], (0, 1), (3, 3)])
    return out


def _forced():
    """The spectrum's table forced to 1,024 slots with 1,100 keys between two small samples: VK_SPEC_TABLE_FULL, no text, a
    zero row, the neighbours exact; and with 900 keys: long probe chains, exact."""
    out = []
    for c in SC.FORCED_CASES:
        out.append(Case(c.name, c.samples, c.k, (1,), [[(0, OPEN), (2, 2), (0, 1)], [(2, OPEN)] * 3], c.slots))
    return out


ALL_CASES = [c for k in KS for c in _cases(k)]
FORCED_CASES = _forced()
BY_NAME = {c.name: c for c in ALL_CASES + FORCED_CASES}

RANDOM_BANDS = [(2, 40), (0, 1), (50, OPEN)]   # of spectrum_cases.random_samples()
