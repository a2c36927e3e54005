"""The rule of `--spectrum-sketch` and `distance` ("`--spectrum-sketch` and `distance`: the rule"), stated
twice: as plain Python loops over sets, and vectorised in NumPy.  Everything is integers; the device equals both exactly.

A table is (keys uint64[nslots], counts uint32[nslots]); a free slot's key is all ones.  A held slot is eligible when its
count is at least m.  The sketch: the min(s, eligible) smallest mix(key) over eligible slots, ascending.  A pair: seen =
min(s, |Sa u Sb|), shared = the values among the seen smallest of Sa u Sb that lie in both."""
import numpy as np

MASK = (1 << 64) - 1
EMPTY = MASK
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def mix(z):
    """splitmix64's finaliser (csrc/vk_screen.h, sc_mix): a bijection on u64."""
    z = ((z ^ (z >> 30)) * C1) & MASK
    z = ((z ^ (z >> 27)) * C2) & MASK
    return z ^ (z >> 31)


def mix_np(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(C1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(C2)
    return z ^ (z >> np.uint64(31))


def sketch_loop(keys, counts, m, s):
    """(sketch as a list of ints, eligible): the loop.  The held keys of a table are distinct (ValueError otherwise)."""
    hashes = set()
    eligible = 0
    for key, count in zip(keys, counts):
        key, count = int(key), int(count)
        if key == EMPTY or count < m:
            continue
        eligible += 1
        h = mix(key)
        if h in hashes:
            raise ValueError("a key lies in two slots")
        hashes.add(h)
    out = []
    while hashes and len(out) < s:
        lowest = min(hashes)
        hashes.remove(lowest)
        out.append(lowest)
    return out, eligible


def sketch_np(keys, counts, m, s):
    """(sketch uint64[length], eligible): vectorised.  (Equal keys in several slots count once per slot here.)"""
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint32)
    ok = (keys != np.uint64(EMPTY)) & (counts >= np.uint32(min(m, 2 ** 32 - 1)))
    h = np.sort(mix_np(keys[ok]))
    return h[:s], int(ok.sum())


def row(sketch, s):
    """A sketch as the device's row: s entries, all ones past its length."""
    out = np.full(s, np.uint64(MASK), dtype=np.uint64)
    out[:len(sketch)] = np.asarray(sketch, dtype=np.uint64)
    return out


def pair_loop(sa, sb, s):
    """(shared, seen) of two sketches made with the same s: the loop."""
    a, b = set(int(x) for x in sa), set(int(x) for x in sb)
    union = sorted(a | b)
    seen = min(s, len(union))
    shared = 0
    for v in union[:seen]:
        if v in a and v in b:
            shared += 1
    return shared, seen


def pair_np(sa, sb, s):
    sa, sb = np.asarray(sa, dtype=np.uint64), np.asarray(sb, dtype=np.uint64)
    union = np.union1d(sa, sb)[:s]
    both = np.intersect1d(sa, sb, assume_unique=True)
    return int(np.isin(union, both, assume_unique=True).sum()), int(len(union))


def bottom(values, s):
    """The s smallest of a set of hashes, ascending: the sketch of the full set."""
    return sorted(values)[:s]


def full_pair(ha, hb, s):
    """(shared, seen) computed from the FULL sets of hashes: the bottom-s of the union, and which of it lies in both.
    pair_loop of the two bottom-s sketches equals it (the property tests/test_sketch_rules.py states)."""
    ha, hb = set(ha), set(hb)
    low = sorted(ha | hb)[:s]
    return sum(1 for v in low if v in ha and v in hb), len(low)
