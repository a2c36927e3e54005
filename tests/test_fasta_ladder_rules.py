"""`image --from-fasta --fragments` without a GPU: the two statements of the rule in tests/fasta_ladder_ref.py agree; the
plan of a 300,000-base sample (names, seeds, thresholds, shifts); the command line; and how far the bases a step takes
may lie from the bases it asks for."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_ladder_ref as LR  # noqa: E402
import fasta_ref as FR  # noqa: E402
from ladder_emit_ref import sample_hash  # noqa: E402


@pytest.mark.parametrize("k", FC.KS)
def test_the_two_statements_agree(k):
    """Through records, pieces, FASTQ and the oracle, and by the byte-at-a-time walk: every small case, every step of
    the GPU test's product (L x threshold x shift x seed)."""
    some = 0
    for name, data in FC.small_cases(k):
        walked = LR.brute_walk(data)
        assert len(walked[0]) == FR.bases(data), name
        for step in LR.steps(k):
            h1, t1 = LR.count(data, k, *step)
            h2, t2 = LR.brute_count(data, k, *step, walked=walked)
            assert t1 == t2, (name, step)
            assert np.array_equal(h1.astype(np.uint64), h2), (name, step)
            some += bool(h1.any())
    assert some > 1000


@pytest.mark.parametrize("k", (5, 9))
def test_every_fragment_taken_still_drops_the_seam_windows(k):
    """Threshold 2^32 is not the whole count: it lacks exactly the windows that lie across a fragment seam."""
    data = FC.fasta([(b"a", FC.seq(1, 1000)), (b"b", FC.seq(2, 333))], 60)
    whole = FR.count(data, k)[0]
    h, taken = LR.count(data, k, 64, 7, LR.ALL, 5)
    assert taken == 1333
    assert (h <= whole).all() and int(whole.sum()) - int(h.sum()) > 15 * (k - 1)
    h0, taken0 = LR.count(data, k, 64, 7, 0, 5)
    assert taken0 == 0 and not h0.any()
    big, _ = LR.count(data, k, 1 << 20, 7, LR.ALL, 0)   # (one fragment holds everything)
    assert np.array_equal(big, whole)


def test_plan_of_300000_bases():
    from varkoder_amd import fasta
    from varkoder_amd.subsample import split_name
    assert [fasta.sample_hash(s, a) for s, a in ((0, 0), (7, 1 << 40), ((1 << 63) + 5, (1 << 64) - 1))] == \
        [sample_hash(s, a) for s, a in ((0, 0), (7, 1 << 40), ((1 << 63) + 5, (1 << 64) - 1))]
    B, L, seed = 300000, 150, 1234567
    recs, steps = fasta.fasta_plan([B], [0], L, seed, min_bp=10000, max_bp=None)   # -m 10K -M 0
    sizes = [300000, 200000, 100000, 50000, 20000, 10000]
    assert [st[2] for st in steps] == sizes
    assert recs[0]["error"] is None and recs[0]["nsites"] == B
    for level, (st, bp) in enumerate(zip(steps, sizes)):
        assert st == (0, level, bp, seed + level, min(1 << 32, bp * (1 << 32) // B),
                      sample_hash(seed + level, (1 << 64) - 1) % L, level == 0)
        assert LR.shift_of(seed + level, L) == st[5]
    assert [fasta.image_name("s", st[2], 7, "cgr") for st in steps] == \
        [split_name("s", bp) + "+cgr+k7.png" for bp in sizes] == \
        ["s@%08dK+cgr+k7.png" % (bp // 1000) for bp in sizes]
    # -M 200K: no whole step; a sample below -m is an error with -M and an empty ladder without; a bad start has no plan
    recs, steps = fasta.fasta_plan([B, 5000, 5000], [0, 0, 1], L, seed, min_bp=10000, max_bp=200000)
    assert [(st[0], st[2], st[6]) for st in steps] == [(0, bp, False) for bp in sizes[1:]]
    assert recs[1]["error"] == "Input file has less than minimum data." and recs[2]["error"]
    recs, steps = fasta.fasta_plan([5000, 0], [0, 0], L, seed, min_bp=10000, max_bp=None)
    assert steps == [] and recs[0]["error"] is None


def test_command_line():
    from varkoder_amd import cli
    plain = cli.parse_args(["image", "in", "--from-fasta"])
    assert sorted(vars(plain)) == ["command", "cpus_per_thread", "from_clean", "from_fasta", "from_raw", "input", "int_folder",
                                   "kmer_mapping", "kmer_size", "label_table", "labels_csv", "max_bp", "min_bp", "n_threads",
                                   "no_adapter", "no_deduplicate", "no_image", "no_merge", "outdir", "overwrite", "seed",
                                   "stats_file", "trim_bp", "verbose"]
    a = cli.parse_args(["image", "in", "--from-fasta", "--fragments"])
    assert a.fragments is True and not hasattr(a, "fragment_length")
    a = cli.parse_args(["image", "in", "--from-fasta", "--fragments", "--fragment-length", "16", "-m", "10K", "-M", "0", "-R", "7"])
    assert a.fragment_length == 16 and cli.max_bp_of(a) is None and cli.parse_size(a.min_bp) == 10000
    assert cli.parse_args(["image", "in", "--from-fasta", "--fragments", "--fragment-length", "1000000"]).fragment_length == 10 ** 6
    for argv in (["image", "in", "--fragments"], ["image", "in", "--from-clean", "--fragments"],
                 ["image", "in", "--fragment-length", "150"], ["image", "in", "--from-raw", "--fragment-length", "150"],
                 ["image", "in", "--from-fasta", "--fragments", "--fragment-length", "15"],
                 ["image", "in", "--from-fasta", "--fragments", "--fragment-length", "1000001"],
                 ["image", "in", "--from-fasta", "--fragments", "--write-splits", "-i", "int"],
                 ["image", "in", "--from-fasta", "--fragments", "--gpu-gzip"],
                 ["query", "in", "out", "-l", "m.pt", "--vocab", "v.txt", "--from-fasta", "--fragments"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv


def taken_bases(B, L, seed, thr, shift):
    """Ordinals of [0, B) in taken fragments, a fragment at a time."""
    f = np.arange(shift // L, (B - 1 + shift) // L + 1, dtype=np.uint64)
    lo = np.maximum(f.astype(np.int64) * L - shift, 0)
    hi = np.minimum((f.astype(np.int64) + 1) * L - shift, B)
    take = LR.hash_array(seed, f) < np.uint64(thr)
    return int((hi - lo)[take].sum()), len(f)


def test_bases_taken_lie_near_the_bases_asked_for():
    """A step of bp bases takes each of the N fragments of a B-base sample with probability p = threshold / 2^32, so the
    number taken is binomial(N, p) with standard deviation sqrt(N p (1 - p)), and the bases taken are L times that (the
    two clipped end fragments aside): |taken - bp| <= 5 L sqrt(N p (1 - p)) -- five standard deviations of a sum that
    is all but normal at these N; nothing here is fitted to what the hash gives."""
    from varkoder_amd.subsample import threshold
    worst = 0.0
    for B in (300000, 1000000):
        for L in (64, 150, 1000):
            for seed in (0, 7, 123456789, (1 << 62) + 11):
                for bp in (B // 2, B // 5, B // 10, B // 50):
                    thr = threshold(bp, B)
                    taken, N = taken_bases(B, L, seed, thr, LR.shift_of(seed, L))
                    p = thr / 2 ** 32
                    bound = 5 * L * math.sqrt(N * p * (1 - p))
                    worst = max(worst, abs(taken - bp) / (bound / 5))
                    assert abs(taken - bp) <= bound, (B, L, seed, bp, taken)
    print("worst deviation: %.2f standard deviations" % worst)
