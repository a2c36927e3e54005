"""The rule of `--kmer-spectrum` (tests/spectrum_ref.py) holds together without a GPU: its two statements agree on every
case of tests/spectrum_cases.py, a row's invariants hold, and the estimator (varkoder_amd/spectrum.py, and the formulas
restated in spectrum_ref.py) finds the coverage, the genome size and the error rate of simulated libraries from the
REFERENCE's spectrum."""
import functools
import json

import numpy as np
import pytest

import spectrum_cases as SC
import spectrum_ref as R
from screen_cases import fq
from varkoder_amd import spectrum as S


def runs():
    for c in SC.ALL_CASES + SC.FORCED_CASES:
        for every in c.everys:
            yield c, every


def test_the_two_statements_agree_on_every_case():
    n = 0
    for c, every in runs():
        for t in c.samples:
            a, b = R.spectrum_loop(t, c.k, every, c.slots), R.spectrum_numpy(t, c.k, every, c.slots)
            assert a[1] == b[1] and list(a[0]) == b[0].tolist(), (c.name, every)
            n += 1
    assert n > 80


def test_a_rows_invariants():
    for c, every in runs():
        for t in c.samples:
            row, status = R.spectrum_numpy(t, c.k, every, c.slots)
            hist = row[R.HIST_AT:].astype(np.int64)
            if status:
                assert not row.any()
                continue
            assert hist.sum() == row[R.DISTINCT] and row[R.TAKEN] <= row[R.WINDOWS] <= row[R.BASES]
            below = int((np.arange(1, 256) * hist[:255]).sum())
            assert below <= row[R.TAKEN] and (hist[255] or below == row[R.TAKEN]), c.name
            if every == 1:
                assert row[R.TAKEN] == row[R.WINDOWS]


def test_the_cases_hold_what_they_are_named_for():
    for k in SC.KS:
        row = lambda name, i=0, every=1: R.spectrum_numpy(SC.BY_NAME["%s_k%d" % (name, k)].samples[i], k, every)   # noqa: E731
        r, _ = row("len_k_minus_1_k_k_plus_1")
        assert r[:5].tolist() == [4, 3 * k, 3, 3, 2]              # (K - 1: none; K: one; K + 1: two, the first shared)
        r, _ = row("bin_edges")
        assert r[R.DISTINCT] == 5 and [int(r[R.HIST_AT + i]) for i in (0, 1, 254, 255)] == [1, 1, 1, 2]
        r, _ = row("poly_a_600")
        assert r[R.HIST_AT + 255] == 1 and r[R.DISTINCT] == 1 + 50 - k + 1
        assert row("poly_a_600", 1)[0][R.HIST_AT:].tolist() == [0] * 255 + [1]      # (T's key is A's)
        r, _ = row("reverse_complement_pairs")
        assert r[R.HIST_AT + 1] == r[R.DISTINCT] == 2 * (75 - k + 1)
        c = SC.BY_NAME["bad_framing_between_good_k%d" % k]
        assert [R.spectrum_numpy(t, k)[1] for t in c.samples] == [0, 1, 0, 2, 1, 0]
        assert [len(R.taken_keys(SC.BY_NAME["random_every_k%d" % k].samples[0], k, e)) > 20 for e in (1, 2, 16)] == [True] * 3
    r, _ = R.spectrum_numpy(SC.BY_NAME["palindrome_16_k16"].samples[0], 16)
    assert r[R.WINDOWS] > r[R.DISTINCT] >= 2
    assert [R.spectrum_numpy(c.samples[1], c.k, 1, c.slots)[1] for c in SC.FORCED_CASES] == [0, R.VK_SPEC_TABLE_FULL]
    assert [int(R.spectrum_numpy(c.samples[1], c.k)[0][R.DISTINCT]) for c in SC.FORCED_CASES] == [900, 1100]
    t = SC.overflow_sample()
    assert R.spectrum_numpy(t, 16, 64)[0][R.DISTINCT] == 3000 > R.slots_for(len(t), 64)


def test_key_sampling_takes_whole_keys():
    """every occurrence of a taken key counts: the sampled spectrum is the whole one restricted to the taken keys"""
    c = SC.BY_NAME["random_every_k21"]
    keys = R.keys_numpy([seq for _, seq in R.screen_ref.split_records(c.samples[0])[1]], 21)
    for every in (2, 16):
        took = R.taken_keys(c.samples[0], 21, every)
        assert all(R.taken(int(x), every) for x in took)
        assert int(R.spectrum_numpy(c.samples[0], 21, every)[0][R.TAKEN]) == int(np.isin(keys, took).sum())
        assert 0 < len(took) < len(np.unique(keys))


# ------------------------------------------------------------------ estimates --

GENOME, LENGTH, ERROR, K = 200000, 150, 0.005, 21
# twice the worst relative deviation over the 15 simulations below, measured on the CPU with the reference's spectrum:
TOL = {"kmer_coverage": 0.105, "genome_kmers": 0.108, "error_rate": 0.29}


@functools.lru_cache(maxsize=None)
def simulated_row(coverage, seed):
    rng = np.random.default_rng(seed)
    row, status = R.spectrum_numpy(fq(SC.simulated_reads(rng, GENOME, coverage * GENOME // LENGTH, LENGTH, ERROR)), K)
    assert status == 0
    return row


@pytest.mark.parametrize("coverage", (2, 8, 30))
def test_the_estimator_on_simulated_libraries(coverage):
    """200 kb random genome, 150-base reads of either strand, 0.5 % substitutions, K = 21, seeds 1..5.  The truth:
    lambda = coverage (L - K + 1) / L (1 - e)^K, G = 200,000 - K + 1 distinct k-mers, error rate 0.005.

    Worst relative deviations measured over the five seeds (lambda, G, error_rate):
        2x   0.052  0.054  0.144      8x   0.040  0.005  0.027      30x   0.024  0.050  0.042
    The tolerance is twice the worst of each over all fifteen: 0.105, 0.108, 0.29."""
    truth = {"kmer_coverage": coverage * (LENGTH - K + 1) / LENGTH * (1 - ERROR) ** K, "genome_kmers": GENOME - K + 1,
             "error_rate": ERROR}
    for seed in range(1, 6):
        row = simulated_row(coverage, seed)
        est, ref = S.estimate(row, K, 1), R.estimate(row, K, 1)
        assert est["reason"] is None and est["support"] == ref["support"] >= S.MIN_SUPPORT
        for name in S.ESTIMATES + ("singleton_fraction",):
            assert est[name] == pytest.approx(ref[name], rel=1e-12), name   # (the product's formulas are the rule's)
        dev = {name: abs(est[name] / truth[name] - 1) for name in TOL}
        print(coverage, seed, {n: round(v, 4) for n, v in dev.items()})
        for name, tol in TOL.items():
            assert dev[name] <= tol, (name, seed, est[name], truth[name])
        assert est["base_coverage"] == pytest.approx(int(row[R.BASES]) / est["genome_kmers"])
        assert 0 <= est["high_copy_fraction"] < 0.01   # (a random genome has no repeats)


def test_key_sampling_scales_the_genome_back():
    """every = 4 on the 8x library: a quarter of the keys, the same coverage, G scaled back by 4"""
    rng = np.random.default_rng(1)
    text = fq(SC.simulated_reads(rng, GENOME, 8 * GENOME // LENGTH, LENGTH, ERROR))
    whole, part = S.estimate(simulated_row(8, 1), K, 1), S.estimate(R.spectrum_numpy(text, K, 4)[0], K, 4)
    assert part["reason"] is None
    # (a quarter of the keys: the sampling error of lambda doubles -- 2 x 0.105 -- and G's with it)
    assert part["kmer_coverage"] == pytest.approx(whole["kmer_coverage"], rel=0.21)
    assert part["genome_kmers"] == pytest.approx(GENOME - K + 1, rel=0.216)


def row_from(hist, every=1):
    row = np.zeros(R.NSTAT, dtype=np.uint64)
    for c, n in hist.items():
        row[R.HIST_AT + c - 1] = n
    row[R.DISTINCT] = sum(hist.values())
    row[R.TAKEN] = row[R.WINDOWS] = sum(c * n for c, n in hist.items())
    row[R.BASES], row[R.READS] = 2 * int(row[R.WINDOWS]), 100
    return row


def test_the_null_branches():
    for est in (S.estimate, R.estimate):
        few = est(row_from({1: 50000, 2: 600, 3: 300}), 21, 1)          # a shallow skim: 900 repeated k-mers behind the mode
        assert few["reason"] == "too few repeated k-mers" and few["support"] == 900
        assert all(few[n] is None for n in S.ESTIMATES) and few["singleton_fraction"] == pytest.approx(50000 / 50900)
        above = est(row_from({1: 100, 254: 2000, 255: 2500, 256: 9000}), 21, 1)   # the peak lies in the overflow bin
        assert above["reason"] == "coverage above the histogram" and all(above[n] is None for n in S.ESTIMATES)
        ok = est(row_from({1: 100, 253: 2000, 254: 2500, 255: 2000, 256: 100}), 21, 1)   # (just below it: estimated)
        assert ok["reason"] is None and ok["kmer_coverage"] is not None
        empty = est(np.zeros(R.NSTAT, dtype=np.uint64), 21, 1)
        assert empty["reason"] == "too few repeated k-mers" and empty["singleton_fraction"] is None


def test_the_report_and_the_columns(tmp_path):
    row = simulated_row(8, 1)
    obj = S.report(row, K, 1)
    assert (obj["k"], obj["every"], obj["reads"], obj["distinct"]) == (K, 1, int(row[R.READS]), int(row[R.DISTINCT]))
    assert obj["histogram"][-1] != 0 and obj["histogram"] == row[R.HIST_AT:R.HIST_AT + len(obj["histogram"])].tolist()
    assert obj["histogram_256_and_more"] == int(row[R.HIST_AT + 255])
    assert obj["estimates"]["reason"] is None and obj["estimates"]["support"] >= 1000
    S.write_report(tmp_path / "d", "s1", obj)
    assert json.loads((tmp_path / "d" / "s1.spectrum.json").read_text()) == obj
    cols = S.columns(row, K, 1)
    assert list(cols) == ["spectrum_kmer_coverage", "spectrum_base_coverage", "spectrum_genome_kmers", "spectrum_error_rate",
                          "spectrum_high_copy_fraction"]
    assert not [c for c in cols if c.endswith("_time")]
    null = S.columns(row_from({1: 10}), K, 1)
    assert list(null) == list(cols) and set(null.values()) == {""}
    assert S.report(row_from({1: 10}), K, 1)["estimates"]["kmer_coverage"] is None
