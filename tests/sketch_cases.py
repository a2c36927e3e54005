"""Inputs for the sketches (tests/sketch_ref.py is the rule): the smallest at which the kernels can go wrong.  Hand-made
tables whose keys are the inverse mix of chosen hashes, so that a case decides which radix rounds run; samples for the
path through the spectrum; pairs of sketches with a common value at every segment seam.  Built on demand, deterministic."""
import random
from collections import namedtuple

import numpy as np

import sketch_ref as R

MASK = R.MASK
INV1, INV2 = pow(R.C1, -1, 1 << 64), pow(R.C2, -1, 1 << 64)   # the two multiplicative inverses of the mix
MIN_SLACK, RUN, DIGIT_BITS = 4096, 2048, 11                   # csrc/vk_sketch.h: kSkMinSlack, kSkRun, kSkDigitBits


def _unshift(z, n):
    x = z
    for _ in range(64 // n + 1):
        x = z ^ (x >> n)
    return x


def unmix(h):
    """The key whose mix is h."""
    z = _unshift(h, 31)
    z = _unshift((z * INV2) & MASK, 27)
    return _unshift((z * INV1) & MASK, 30)


def cap_of(nslots, s):
    """Hashes of the device's candidate buffer for a table of nslots (vkimg.hip, sk_cap)."""
    return -(-(s + max(MIN_SLACK, nslots >> DIGIT_BITS)) // RUN) * RUN


Table = namedtuple("Table", "name keys counts m s")


def make_table(name, nslots, hashes, counts, m, s, seed=1):
    """A table of nslots with the keys of these hashes at random slots, every other slot free."""
    assert len(hashes) == len(counts) <= nslots
    keys = [unmix(h) for h in hashes]
    assert all(R.mix(k) == h and k != MASK for k, h in zip(keys, hashes))   # (the round trip; never a key of all ones)
    at = random.Random(seed).sample(range(nslots), len(keys))
    k = np.full(nslots, np.uint64(MASK), dtype=np.uint64)
    c = np.zeros(nslots, dtype=np.uint32)
    k[at] = np.array(keys, dtype=np.uint64)
    c[at] = np.array(counts, dtype=np.uint32)
    return Table(name, k, c, m, s)


def spread(rng, n, top=0, top_bits=0):
    """n distinct hashes whose top `top_bits` bits are `top`, the rest random."""
    out = set()
    while len(out) < n:
        out.add((top << (64 - top_bits)) | rng.getrandbits(64 - top_bits) if top_bits else rng.getrandbits(64))
    out.discard(MASK)
    return sorted(out)


SEAM = 16384 + 1024   # slots: two workgroups of the table passes


def hand_tables():
    """The hand-made tables of the GPU tests (and, with smaller buffers, of the emulation)."""
    rng = random.Random(2024)
    out = []
    h = spread(rng, 500)
    out.append(make_table("1024_slots_all_candidates", 1024, h, [1] * 500, 1, 64))
    out.append(make_table("1024_slots_fewer_than_s", 1024, h[:40], [1] * 40, 1, 64))
    out.append(make_table("1024_slots_none", 1024, [], [], 1, 64))
    # more eligible than the buffer holds (64 + 4,096 -> 6,144): the select runs
    assert cap_of(SEAM, 64) == 6144
    h = spread(rng, 9000)
    out.append(make_table("seam_spread", SEAM, h, [1] * 9000, 1, 64))
    out.append(make_table("seam_spread_s_2049", SEAM, h, [1] * 9000, 1, 2049))
    for bits in (11, 22, 33, 44):   # a crossing bin that holds ALL the eligible keys, round after round
        h = spread(rng, 9000, top=rng.getrandbits(bits), top_bits=bits)
        out.append(make_table("seam_shared_top_%d" % bits, SEAM, h, [1] * 9000, 1, 64))
    # a crossing bin that holds ONE: 63 hashes in bin 0, one in bin 1, the rest from bin 2 up
    low = spread(rng, 63, top=0, top_bits=11) + spread(rng, 1, top=1, top_bits=11)
    high = [x for x in spread(rng, 9000) if x >> 53 >= 2]
    out.append(make_table("seam_crossing_bin_of_one", SEAM, low + high, [1] * (64 + len(high)), 1, 64))
    # multiplicities m - 1 and m
    h = spread(rng, 9000)
    for m in (1, 2, 3):
        counts = [m - 1 if i % 3 == 0 else m if i % 3 == 1 else m + 5 for i in range(9000)]
        out.append(make_table("seam_min_count_%d" % m, SEAM, h, counts, m, 64))
    # an s just above the run length, the candidates four runs: two merge levels
    assert cap_of(SEAM, RUN + 1) == 4 * RUN
    h = spread(rng, 7000)
    out.append(make_table("two_merge_levels", SEAM, h, [2] * 7000, 2, RUN + 1))
    out.append(make_table("two_merge_levels_s_above_eligible", SEAM, h, [2] * 7000, 1, 7500))
    return out


def big_table():
    """s = 2^20 with only 2,000 eligible."""
    rng = random.Random(99)
    return make_table("s_2_20_eligible_2000", 4096, spread(rng, 2000), [1] * 2000, 1, 1 << 20)


def duplicate_table():
    """A key in 7,000 slots, and 100 others around it: outside the rule's tables (held keys are distinct), inside the
    device's bound -- every round runs, and its hash counts once per slot (sketch_ref.sketch_np)."""
    rng = random.Random(5)
    mid = 1 << 63
    h = [x for x in spread(rng, 100) if x != mid]
    return make_table("one_key_in_7000_slots", SEAM, h + [mid] * 7000, [1] * (len(h) + 7000), 1, 2000)


# ---------------------------------------------------------------------- pairs --

def seam_pairs(s=64):
    """(name, A, B): pairs of sketches of size s.  With la + lb = n a lane's segment is ceil(n / 64) merged values: the
    common values are placed so that a duplicate pair straddles each seam."""
    rng = random.Random(31)
    out = []
    full = spread(rng, 3 * s)
    a, b = full[0:2 * s:2], full[1:2 * s:2]              # interleaved, disjoint
    out += [("empty_empty", [], []), ("empty_one", [], full[:1]), ("one_one_same", full[:1], full[:1]),
            ("one_one_differ", full[:1], full[1:2]), ("identical_full", a, a), ("disjoint_full", a, b),
            ("disjoint_blocks", full[:s], full[s:2 * s]), ("s_minus_1_and_s", a[:s - 1], sorted(a[:s // 2] + b[:s - s // 2])),
            ("full_and_empty", a, []), ("one_in_full", a, [a[s // 2]])]
    # every second value common
    out.append(("interleaved_half_common", a, sorted(a[::2] + b[::2])))
    # la + lb no multiple of 64, and a common value at EVERY seam: with segments of `seg` merged values, make the merged
    # list so that positions seg - 1 and seg (and 2 seg - 1, 2 seg, ...) are the two copies of one value
    for la, lb in ((s, s - 3), (s - 1, s // 2 + 5), (37, 30)):
        n = la + lb
        seg = -(-n // 64)
        vals = iter(spread(rng, 2 * n))
        A, B = [], []
        pos = 0
        while len(A) < la or len(B) < lb:
            v = next(vals)
            at_seam = seg > 0 and (pos + 1) % seg == 0
            if at_seam and len(A) < la and len(B) < lb:
                A.append(v)
                B.append(v)
                pos += 2
            elif len(A) < la and (len(B) >= lb or rng.random() < 0.5):
                A.append(v)
                pos += 1
            else:
                B.append(v)
                pos += 1
        out.append(("common_at_seams_%d_%d" % (la, lb), A, B))
    return out


def pair_rows(sketches, s):
    """(rows uint64[n, s], lengths uint64[n]) of a list of sketches."""
    rows = np.stack([R.row(x, s) for x in sketches]) if sketches else np.zeros((0, s), dtype=np.uint64)
    return rows, np.array([len(x) for x in sketches], dtype=np.uint64)
