"""Adapters by sequence at their boundaries: seeded builders that the CPU tests (test_adapter_rules.py), the host
emulation (test_adapter_emulation.py) and the GPU tests (test_gpu_adapter_edges.py) share, after clean_cases.py.

A builder returns a clean_cases batch (texts, roles, owner, records, nsamples) with the expected result written down
in it.  trim_sweep(): one sample per adapter length 1..64 (and further samples with non-ACGT adapters and with pairs)
whose reads put the adapter at every kind of place; "adapters" is the table, "census" the share of reads that end
uncut, cut to nothing and cut in between.  detect_edges(): one group per boundary of the detection rule, every group
the single reads of a sample of its own; "planted"[T][sample] is the adapter that the rule must find with the tail
trim T (FREE: not written down for that T, the reference alone decides), "reads"[sample] the group's evaluation set
and "names" the samples by what they test.  Every constant comes from adapter_ref.py or adapters.py.  Tests only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_ref as A  # noqa: E402
import clean_cases as K  # noqa: E402
import clean_ref as R  # noqa: E402

from varkoder_amd import adapters as table  # noqa: E402

SEED = b"ACGTTGCATC"                     # a fixed 10-mer that passes key_ok
FREE = "not planted"                     # planted[T][j] of a group whose result at T nobody wrote down
TS = (0, 1, 10, 25)                      # the tail trims that detection is run with
ASSERTED = (7, 8, 11, 12, 15, 16, 31, 32, 33, 63, 64)   # adapter lengths the tests look at one by one
MAX_ADAPTER = 64
NEXTERA = dict(table.KNOWN_ADAPTERS)["Nextera / Tn5"]
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def key_of(kmer):
    return sum(b"ACGT".index(c) << (2 * (A.SEED_K - 1 - i)) for i, c in enumerate(kmer))


def _other(rng, b):
    """A base that differs from byte b."""
    return int(rng.choice([c for c in b"ACGT" if c != b]))


# --------------------------------------------------------------- trim sweep ---

def _mismatched(rng, piece, k, forced):
    """piece with exactly k bases changed, at the positions `forced` first (those inside the piece), then anywhere."""
    s = bytearray(piece)
    at = [i for i in dict.fromkeys(forced) if 0 <= i < len(s)][:k]
    rest = [i for i in rng.permutation(len(s)) if i not in at]
    for i in at + [int(i) for i in rest[:k - len(at)]]:
        s[i] = _other(rng, s[i])
    return bytes(s)


def _sweep_reads(rng, ad, n=200):
    """About n read sequences around the adapter `ad`: insert + a piece of the adapter + a tail or none."""
    L = len(ad)
    start = -A.trim_start(L)
    out = []

    def seq(k):
        return R._rng_seq(rng, int(k))

    for r in range(6):                                   # reads of 0..5 bases: nothing is ever compared
        out.append(seq(r) if r % 2 else ad[:r])
    for h in range(7):                                   # dimers: the adapter at position 0 without its first h bases
        for _ in range(4):
            out.append(ad[h:] + seq(rng.integers(0, 90)))
        out.append(ad[h:])
    for h in (start + 1, 0):                             # ... behind a few bases of insert
        for k in (1, 2, 3):
            out.append(seq(k) + ad[h:] + seq(rng.integers(5, 60)))
    for left in (4, 5, 6):                               # exactly 4 (never tried), 5 and 6 bases left at the read's end
        for _ in range(3):
            out.append(seq(rng.integers(0, 151)) + ad[:left])
    while len(out) < n:
        kind = len(out) % 8
        ins = seq(rng.integers(0, 151))
        if kind == 0:                                    # read through into a random tail
            out.append(ins + ad + seq(rng.integers(0, 50)))
        elif kind == 1:                                  # cut anywhere
            out.append(ins + ad[:int(rng.integers(1, L + 1))])
        elif kind in (2, 3):                             # exactly cmplen // 8 (kind 2) or one more (3) mismatches
            c = L if rng.random() < 0.5 else int(rng.integers(min(5, L), L + 1))
            forced = [(0, c - 1), (31, 32), (32, 0), (c - 1, 31), ()][int(rng.integers(0, 5))]
            piece = _mismatched(rng, ad[:c], c // 8 + (kind == 3), forced)
            out.append(ins + piece + (seq(rng.integers(0, 40)) if c == L else b""))
        elif kind == 4:                                  # non-ACGT bytes in the read, inside and around the adapter
            s = bytearray(ins + ad + seq(rng.integers(0, 30)))
            for i in rng.integers(0, len(s), int(rng.integers(1, 4))):
                s[i] = (ord("N"), s[i] | 0x20, ord("."))[int(rng.integers(0, 3))]
            out.append(bytes(s))
        elif kind == 5:                                  # no adapter at all
            out.append(ins)
        elif kind == 6:                                  # a dimer with a mismatch budget spent at its ends
            c = L - int(rng.integers(0, min(start, L - 1) + 1))
            piece = ad[L - c:]
            out.append(_mismatched(rng, piece, len(piece) // 8 + int(rng.integers(0, 2)), (0, len(piece) - 1))
                       + seq(rng.integers(0, 70)))
        else:                                            # the adapter twice: the first place wins
            out.append(ins + ad[:int(rng.integers(5, L + 5))] + seq(3) + ad)
    return out


def _faced(rng, ad, marks):
    """Reads for an adapter with non-ACGT bytes at `marks`: the same byte in the read, another non-ACGT byte, a base."""
    out = []
    for _ in range(12):
        for how in range(4):
            s = bytearray(ad)
            for i in marks:
                if how == 1:
                    s[i] = ord("N") if s[i] != ord("N") else ord("n")
                elif how == 2:
                    s[i] = _other(rng, s[i])
                elif how == 3 and i == marks[0]:
                    s[i] = ord(".") if s[i] != ord(".") else ord("N")
            out.append(R._rng_seq(rng, int(rng.integers(0, 120))) + bytes(s) + R._rng_seq(rng, int(rng.integers(0, 30))))
    return out


def _records(rng, tag, seqs):
    return [(b"@%s.%d" % (tag, i), s, R._qual(rng, len(s))) for i, s in enumerate(seqs)]


def census_of(pairs):
    """[uncut, cut to nothing, cut in between] of (read, adapter) pairs under adapter_ref's rule."""
    c = [0, 0, 0]
    for s, ad in pairs:
        n = A.trim_by_sequence(s, ad)
        c[0 if n == len(s) else 1 if n == 0 else 2] += 1
    return c


@functools.lru_cache(maxsize=None)
def trim_sweep():
    """The batch (F = T = 0, dedup off, adapter trimming on).  Samples 0..63: single reads, adapter length sample + 1.
    "dirty": {length: sample} with N / lower case / '.' in the adapter; "pairs": [(sample, len R1's, len R2's)];
    "cases": every (read, adapter) that meets the rule, as sequences; "census": their three classes."""
    rng = np.random.default_rng(8101)
    b = K.Batch()
    b["adapters"], b["cases"], b["dirty"], b["pairs"] = [], [], {}, []
    for L in range(1, MAX_ADAPTER + 1):
        ad = R._rng_seq(rng, L)
        seqs = _sweep_reads(rng, ad)
        b.add_sample([], [], _records(rng, b"a%d" % L, seqs))
        b["adapters"].append([None, None, ad])
        b["cases"] += [(s, ad) for s in seqs]
    for L in ASSERTED:
        s = bytearray(R._rng_seq(rng, L))
        marks = sorted({L // 3, min(L - 1, 32), L - 1})
        for i, m in zip(marks, b"Nn."):
            s[i] = m
        ad = bytes(s)
        seqs = _sweep_reads(rng, ad, 120) + _faced(rng, ad, marks)
        b["dirty"][L] = b.add_sample([], [], _records(rng, b"n%d" % L, seqs))
        b["adapters"].append([None, None, ad])
        b["cases"] += [(s, ad) for s in seqs]
    for l1, l2 in ((7, 33), (8, 12), (16, 64), (31, 32), (63, 15), (11, 64), (33, 7), (12, 16), (64, 8), (32, 11)):
        # (no G in what follows an insert: the poly-G trim ahead of this step ends where the G pad starts)
        a1, a2 = R._rng_seq(rng, l1, b"ACT"), R._rng_seq(rng, l2, b"ACT")
        r1, r2 = [], []
        for p in range(60):
            ins = R._rng_seq(rng, int(rng.integers(0, 30)) if p % 4 else 0)   # (under the overlap's 30)
            # p % 5 == 1 / 2: R2 / R1 runs into something that is not its adapter, so that mate alone is kept
            x, y = R.pair_from_insert(rng, b"p%d_%d.%d" % (l1, l2, p), ins, 100,
                                      R._rng_seq(rng, 40, b"ACT") if p % 5 == 2 else a1,
                                      R._rng_seq(rng, 40, b"ACT") if p % 5 == 1 else a2)
            r1.append(x)
            r2.append(y)
        b["pairs"].append((b.add_sample(r1, r2, []), l1, l2))
        b["adapters"].append([a1, a2, None])
        b["cases"] += [(R._trim(x, 0, 0)[1], a1) for x in r1] + [(R._trim(y, 0, 0)[1], a2) for y in r2]
    b["census"] = census_of(b["cases"])
    return b


@functools.lru_cache(maxsize=None)
def sweep_expected(merge=True):
    """[(text, stats words, status, [reads, bases] cut by sequence)] per sample of trim_sweep()."""
    b = trim_sweep()
    out = []
    for (r1, r2, se, status), t in zip(K.groups(b), b["adapters"]):
        assert status == 0
        text, st, ad = A.clean_sample_adapters(r1, r2, se, F=0, T=0, adapter=True, merge=merge, dedup=False, adapters=t)
        out.append((text, K.stats_words(st), 0, [ad["reads"], ad["bases"]]))
    return out


# ----------------------------------------------------------------- detection ---

def _text(tag, seqs):
    """FASTQ text of the sequences, headers and qualities of no interest."""
    return b"".join(b"@%s.%d\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def _random_reads(rng, n, L):
    m = _ACGT[rng.integers(0, 4, (n, L))]
    return [row.tobytes() for row in m]


class _Groups:
    """detect_edges() under construction: a group is the single reads of the next sample."""

    def __init__(self):
        self.b = K.Batch()
        self.b.update(planted={T: [] for T in TS}, reads=[], names={}, large=[], budgets={})

    def add(self, name, files, want, records=None):
        """files: lists of sequences, in file order; want: the planted adapter, or {T: adapter} (a T left out: FREE);
        records: the files' budgets (None: all).  Returns the sample."""
        b = self.b
        j = b["nsamples"]
        b["nsamples"] += 1
        seqs = []
        for i, f in enumerate(files):
            b.add(_text(b"%s_%d" % (name.encode(), i), f), K.SE, j, None if records is None else records[i])
            seqs += f if records is None else f[:records[i]]
        b["reads"].append(seqs[:A.EVAL_RECORDS])
        for T in TS:
            b["planted"][T].append(want.get(T, FREE) if isinstance(want, dict) else want)
        b["names"][name] = j
        return j

    def empty_sample(self, name):
        """A sample with no files at all."""
        j = self.b["nsamples"]
        self.b["nsamples"] += 1
        self.b["reads"].append([])
        for T in TS:
            self.b["planted"][T].append(None)
        self.b["names"][name] = j
        return j


def _shift(T):
    return max(1, T)


def _seeded_read(rng, n, p, tries=200):
    """A read of n random bases whose lexicographically first window that passes the key filters (the first candidate
    of a set of identical reads: every window counts alike) starts at p."""
    small = b"AAAAACCCGT"
    for _ in range(tries):
        s = bytearray(R._rng_seq(rng, n))
        s[p:p + A.SEED_K] = small
        cands, _ = A.candidates([bytes(s)] * A.MIN_VOTES)
        if cands and bytes(s).find(A.key_str(cands[0][0]), A.SEED_FROM) == p and bytes(s).count(small) == 1:
            return bytes(s)
    raise AssertionError("no such read")


def fold_sets(rng, P):
    """(at, over): the reads of the two fold groups.  `at`: 50 reads P + SEED + G among random 40-base reads without
    SEED and one-window fillers, so that `total` (the count sum of every key that passes the filters) is exactly
    50 * 4^10 // (FOLD + 1): count * 4^10 // total is FOLD + 1.  `over`: one filler more, FOLD."""
    target = A.MIN_VOTES * 4 ** A.SEED_K // (A.FOLD + 1)
    ok = A.key_ok()
    nxt = (SEED + b"G")[1:]
    bg = [s for s in _random_reads(rng, 256650, 40) if SEED not in s and nxt not in s]
    reads = bg + [P + SEED + b"G"] * A.MIN_VOTES
    m = np.frombuffer(b"".join(bg), dtype=np.uint8).reshape(len(bg), 40)
    key, valid = A._windows(np.concatenate([m, np.zeros((len(bg), 1), dtype=np.uint8)], axis=1))
    valid[:, :A.SEED_FROM] = False
    total = int(ok[key[valid]].sum()) + 2 * A.MIN_VOTES        # (SEED and nxt pass the filters)
    assert ok[key_of(SEED)] and ok[key_of(nxt)] and total <= target
    keys = np.flatnonzero(ok)
    keys = keys[(keys != key_of(SEED)) & (keys != key_of(nxt))]
    pick = keys[rng.integers(0, len(keys), target - total + 1)]
    head = _random_reads(rng, len(pick), A.SEED_FROM)
    fill = [h + A.key_str(int(k)) for h, k in zip(head, pick)]     # 30 bases: one counted window, p = 20
    assert len(reads) + len(fill) <= A.EVAL_RECORDS
    return reads + fill[:-1], reads + fill


@functools.lru_cache(maxsize=None)
def detect_edges():
    rng = np.random.default_rng(8201)
    g = _Groups()
    b = g.b
    U = R._rng_seq(np.random.default_rng(8202), 80)
    P = R._rng_seq(np.random.default_rng(8203), A.SEED_FROM)
    b["U"], b["P"] = U, P
    dimer = U[:70]
    reach = {T: U[:min(A.MAX_DETECTED, len(dimer) - _shift(T))] for T in TS}
    bg = [s for s in _random_reads(rng, 2000, 60)      # (no read holds a 10-mer of the dimer by accident)
          if not any(dimer[i:i + A.SEED_K] in s for i in range(len(dimer) - A.SEED_K + 1))]

    # no candidates, ahead of everything else (the first slice)
    g.add("short", [[R._rng_seq(rng, int(rng.integers(0, 30))) for _ in range(300)]], None)
    g.add("poly", [[b"A" * 80, b"G" * 80, b"A" * 10 + b"G" * 70] * 40], None)
    g.add("all_n", [[b"N" * 70] * 120], None)
    g.add("zero_records", [[]], None)
    g.add("zero_budget", [[dimer] * 80], None, records=[0])
    g.empty_sample("no_files")

    # votes: MIN_VOTES occurrences, and one fewer
    g.add("votes_at", [bg + [dimer] * A.MIN_VOTES], reach)
    g.add("votes_under", [bg + [dimer] * (A.MIN_VOTES - 1)], None)

    # consensus: 100 reads, CONSENSUS_PCT of them agree at base 45, and one fewer
    def changed(n_agree):
        bad = bytearray(dimer)
        bad[45] = _other(rng, bad[45])
        return [dimer] * n_agree + [bytes(bad)] * (100 - n_agree)
    g.add("consensus_at", [changed(A.CONSENSUS_PCT)], {T: reach[T] for T in (0, 1, 10)})
    g.add("consensus_under", [changed(A.CONSENSUS_PCT - 1)], {T: None for T in (0, 1, 10)})

    # the reach of T
    g.add("reach", [[dimer] * 60], reach)

    # the first counted position and the tail's limit, for reads made for the shift sb = max(1, T) of T = 0 / 1 and 10;
    # run with another T the result is left to the reference
    b["first_position"] = {}
    for sb in (1, 10):
        tail = R._rng_seq(np.random.default_rng(8204), sb)
        full = P + SEED + tail
        at = [T for T in TS if _shift(T) == sb]
        names = {}
        names["all"] = g.add(f"first_{sb}_all", [[full] * A.MIN_VOTES], {T: P + SEED for T in at})
        names["p19"] = g.add(f"first_{sb}_p19", [[full] * (A.MIN_VOTES - 1) + [P[1:] + SEED + tail + b"A"]], {T: None for T in at})
        names["short_tail"] = g.add(f"first_{sb}_short_tail", [[full] * (A.MIN_VOTES - 1) + [full[:-1]]], {T: None for T in at})
        names["long_tail"] = g.add(f"first_{sb}_long_tail", [[full] * (A.MIN_VOTES - 1) + [full + b"C"]], {T: P + SEED for T in at})
        b["first_position"][sb] = names

    # snapping on the last SNAP_BASES bytes of the 60 kept, and one byte later
    b["snap"] = {}
    for name, ad in (("truseq1", A.TRUSEQ1), ("nextera", NEXTERA)):
        for nx in (A.MAX_DETECTED - table.SNAP_BASES, A.MAX_DETECTED - table.SNAP_BASES + 1):
            read = R._rng_seq(rng, nx) + ad + R._rng_seq(rng, 20)
            D = {T: read[:min(A.MAX_DETECTED, len(read) - _shift(T))] for T in TS}   # (identical reads: all of a read's reach)
            want = {T: ad if ad[:table.SNAP_BASES] in D[T] else D[T] for T in TS}
            assert want[10] == (ad if nx + table.SNAP_BASES <= A.MAX_DETECTED else read[:A.MAX_DETECTED])
            b["snap"][(name, nx)] = g.add(f"snap_{name}_{nx}", [[read] * 60], want)

    # the backward ring wraps (the first candidate at p = 70); more than 64 forward steps (at p = 20)
    for name, p in (("ring", 70), ("cap", A.SEED_FROM)):
        read = _seeded_read(rng, 150, p)
        g.add(name, [[read] * 60], read[:A.MAX_DETECTED])

    # a consensus that holds N
    s = bytearray(R._rng_seq(rng, 80))
    s[15] = s[50] = ord("N")
    g.add("with_n", [[bytes(s)] * 60], {T: bytes(s)[:min(A.MAX_DETECTED, 80 - _shift(T))] for T in TS})

    # the fold threshold at its boundary (large)
    at, over = fold_sets(rng, P)
    b["large"].append(g.add("fold_at", [at], {0: P + SEED, 1: P + SEED, 10: None, 25: None}))
    b["large"].append(g.add("fold_over", [over], None))

    # the evaluation set: EVAL_RECORDS records over two files, the last 50 / 49 of them dimers (large); with budgets
    # that end as many dimers into file 2 well below EVAL_RECORDS, the same answers
    for n, name in ((A.MIN_VOTES, "eval_at"), (A.MIN_VOTES - 1, "eval_under")):
        f1 = _random_reads(rng, 200000, 30)
        nbg = A.EVAL_RECORDS - n - len(f1)
        f2 = _random_reads(rng, nbg, 30) + [dimer] * 100
        j = g.add(name, [f1, f2], reach if n == A.MIN_VOTES else None)
        b["large"].append(j)
        b["budgets"][j] = [100000, nbg + n]

    # ten equal counts ranked across threads: 49,932 distinct keys once each
    ok = np.flatnonzero(A.key_ok())[::7][:49932]
    head = R._rng_seq(np.random.default_rng(0), A.SEED_FROM)
    g.add("ties", [[head + A.key_str(int(k)) for k in ok]], None)

    # further small groups: more than 32 groups with records, no-candidate groups on both sides of the slice boundary
    small_rna = dict(table.KNOWN_ADAPTERS)["Illumina small RNA 3'"]
    for i, ad in enumerate((A.TRUSEQ2, small_rna, A.TRUSEQ1)):
        reads = [s for _, s, _ in A.se_readthrough(8300 + i, 600, 0.3, adapter=ad, L=100, insert=(25, 60))]
        g.add(f"more_{i}", [reads], {10: ad})
        g.add(f"none_{i}", [[R._rng_seq(rng, int(rng.integers(0, 30))) for _ in range(40)] + [b"N" * 90] * 60], None)
    g.add("last_poly", [[b"G" * 60, b"A" * 60] * 50], None)
    return b


def active_groups(b, records=None):
    """The samples of a detect_edges batch whose group has records, in the order detection takes them."""
    rec = b["records"] if records is None else records
    have = [0] * b["nsamples"]
    for j, n in zip(b["owner"], rec):
        have[j] += n
    return [j for j in range(b["nsamples"]) if have[j]]


def budget_records(b):
    """(records, evaluation sets, planted at T = 10) of detect_edges() with the budgets of the two evaluation-set
    groups in place: every other group as before."""
    rec = list(b["records"])
    reads = list(b["reads"])
    for j, budget in b["budgets"].items():
        files = [i for i, o in enumerate(b["owner"]) if o == j]
        whole = b["reads"][j]
        n1 = rec[files[0]]
        reads[j] = whole[:budget[0]] + whole[n1:n1 + budget[1]]
        for i, n in zip(files, budget):
            rec[i] = n
    return rec, reads, b["planted"][10]
