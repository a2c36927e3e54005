"""Inputs for the k-mer spectrum (tests/spectrum_ref.py is the rule): the smallest at which the kernels can go wrong, each
at K = 16, 21 and 31.  A case is one call: its samples, K, the values of `every` to run it with, and the forced table
size (None: the engine's).  Built once at import, deterministic."""
import random
from collections import namedtuple

import numpy as np

import screen_ref
import spectrum_ref as R
from screen_cases import fq, rc, seq

Case = namedtuple("Case", "name samples k everys slots")

TILE = 128   # VKIMG_SPECTRUM_TILE of the small-tile runs
KS = (16, 21, 31)


def distinct_kmers(rng, n, k, every=1):
    """n distinct reads of k bases with n distinct keys, every one taken at `every`, none the reverse complement of another."""
    out, seen = [], set()
    while len(out) < n:
        s = seq(rng, k)
        key = screen_ref.key_of(s)
        if key not in seen and R.taken(key, every):
            seen.add(key)
            out.append(s)
    return out


def _cases(k):
    rng = random.Random(1000 + k)
    out = []

    def add(name, samples, everys=(1,), slots=None):
        out.append(Case("%s_k%d" % (name, k), [bytes(s) for s in samples], k, tuple(everys), slots))

    add("empty_sample", [b"", fq([seq(rng, 40)]), b""])
    base = seq(rng, 80)
    add("len_k_minus_1_k_k_plus_1", [fq([base[:k - 1], b"", base[:k], base[:k + 1]])])
    n_mid = bytearray(seq(rng, 90))
    n_mid[45] = ord("N")
    n_at_k = bytearray(seq(rng, 90))
    n_at_k[k] = ord("N")             # (the first window is whole, the next K are broken)
    n_first = bytearray(seq(rng, 90))
    n_first[k - 1] = ord("n")        # (no window before base K)
    add("n_breaks_windows", [fq([bytes(n_mid), bytes(n_at_k), bytes(n_first), b"N" * 50, b"ACGTRYKM" * 10])])
    low = seq(rng, 70)
    add("lower_case", [fq([low.lower(), low, rc(low).lower()])])
    add("crlf", [fq([seq(rng, 60), seq(rng, 33)], eol=b"\r\n")])
    add("no_final_newline", [fq([seq(rng, 60), seq(rng, 50)], last_eol=False)])
    # a read longer than the tile: the window at base TILE - 8 lies across the first seam, and comes again alone
    long_read = seq(rng, 3 * TILE + 17)
    seam = long_read[TILE - 8:TILE - 8 + k]
    add("tile_seam", [fq([long_read, seam, rc(seam), long_read[2 * TILE - k + 1:2 * TILE + 9]])])
    a, b = seq(rng, 75), seq(rng, 75)
    add("reverse_complement_pairs", [fq([a, rc(a), b, rc(b).lower()])])
    add("palindrome_16", [fq([b"ACGT" * 4, b"ACGT" * 4, b"GAATTC" * 6, seq(rng, 5) + b"ACGT" * 4 + seq(rng, 5)])])
    # multiplicities at the histogram's bin edges: reads of exactly K bases, a key each
    mers = distinct_kmers(rng, 5, k)
    reads = []
    for s, m in zip(mers, (1, 2, 255, 256, 257)):
        reads += [s if i % 3 else rc(s) for i in range(m)]
    rng.shuffle(reads)
    add("bin_edges", [fq(reads)])
    add("poly_a_600", [fq([b"A" * 600, seq(rng, 50)]), fq([b"T" * 600]), fq([b"ACGT" * 150, b"AC" * 200])])
    shared = fq([seq(rng, 120), seq(rng, 64)])
    add("two_samples_share_every_kmer", [shared, shared])
    good = fq([seq(rng, 100), seq(rng, 90)])
    add("bad_framing_between_good", [good, good[1:], good, good + b"@x\nACGT\n", good.replace(b"\n+\n", b"\n-\n", 1), good])
    genome = seq(rng, 3000)
    rnd = []
    for _ in range(300):
        at = rng.randrange(len(genome) - 100)
        r = genome[at:at + 100]
        rnd.append(rc(r) if rng.random() < 0.5 else r)
    add("random_every", [fq(rnd)], everys=(1, 2, 16))
    return out


def _forced():
    """K = 21, a table forced to 1,024 slots: about 900 distinct keys (long probe chains, wrap-around at the table's end)
    between two small samples, and about 1,100 (no slot left: VK_SPEC_TABLE_FULL, the neighbours exact)."""
    rng = random.Random(77)
    k = 21
    small = fq([seq(rng, 60), seq(rng, 45)])
    out = []
    for n in (900, 1100):
        mers = distinct_kmers(rng, n, k)
        reads = mers + [rc(s) for s in mers[:n // 3]]   # (a third of the keys twice)
        out.append(Case("forced_1024_slots_%d_keys" % n, [small, fq(reads), small], k, (1,), 1024))
    return out


def overflow_sample(k=16, every=64, n=3000):
    """A sample built to overflow its first table at every > 1: one read of n k-mers whose keys are ALL taken at `every`,
    an N between them, and an empty quality line, so that the text is short and the table the engine gives it
    (spectrum_ref.slots_for) holds fewer slots than the sample has taken keys."""
    rng = random.Random(4242)
    mers = distinct_kmers(rng, n, k, every)
    text = b"@overflow\n" + b"N".join(mers) + b"\n+\n\n"
    assert R.slots_for(len(text), every) < n <= R.slots_for(len(text), 1) // 2
    return text


ALL_CASES = [c for k in KS for c in _cases(k)]
FORCED_CASES = _forced()
BY_NAME = {c.name: c for c in ALL_CASES + FORCED_CASES}


def simulated_reads(rng, genome, reads, length=150, error=0.005):
    """`reads` reads of `length` bases from a random genome of `genome` bases (rng: a numpy Generator), either strand,
    every base substituted with probability `error`: a list of bytes."""
    comp = np.array([3, 2, 1, 0], dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    g = rng.integers(0, 4, genome, dtype=np.uint8)
    at = rng.integers(0, genome - length + 1, reads)
    r = g[at[:, None] + np.arange(length)[None, :]]
    flip = rng.random(reads) < 0.5
    r[flip] = comp[r[flip][:, ::-1]]
    err = rng.random(r.shape) < error
    r[err] = (r[err] + rng.integers(1, 4, int(err.sum()), dtype=np.uint8)) & 3
    return [x.tobytes() for x in letters[r]]


def random_samples(seed=5, reads=20000, length=150, genome=50000, error=0.01):
    """Three samples of `reads` reads from random genomes with substitutions, both strands; the last a quarter poly-A."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(3):
        rows = simulated_reads(rng, genome, reads, length, error)
        if s == 2:
            for i in range(0, reads, 4):
                rows[i] = b"A" * length
        out.append(fq(rows))
    return out
