"""The rule of `--genome-spectrum` (tests/fasta_spectrum_ref.py): its two statements against each other on every case,
against the screen's keys and windows and `--from-fasta`'s bases, the assembly's estimates and report, the per-sample form
of the corrected distance, and the distance between an assembly and simulated libraries of a diverged copy."""
import functools
import json
import random

import numpy as np
import pytest

import fasta_ref
import fasta_spectrum_cases as FC
import fasta_spectrum_ref as FR
import screen_ref
import sketch_ref as R
import spectrum_ref as SR
import test_sketch_rules as TSR
from varkoder_amd import distance, sketch, spectrum


@pytest.mark.parametrize("every", FC.EVERIES)
@pytest.mark.parametrize("k", FC.KS)
def test_the_two_statements_agree_on_every_case(k, every):
    for name, text in FC.cases(k):
        row1, st1, counts1 = FR.spectrum_strings(text, k, every)
        row2, st2, uniq, mult = FR.spectrum_numpy(text, k, every)
        assert st1 == st2 == (1 if name == "bad_start" else 0), name
        assert list(map(int, row2)) == row1, name
        assert dict(zip(uniq.tolist(), mult.tolist())) == counts1, name
        assert sum(row1[FR.HIST_AT:]) == row1[FR.DISTINCT] and row1[FR.TAKEN] <= row1[FR.WINDOWS], name


@pytest.mark.parametrize("k", FC.KS)
def test_keys_and_windows_are_the_screens_and_bases_the_counts(k):
    for name, text in FC.cases(k):
        row, st, counts = FR.spectrum_strings(text, k, 1)
        if st:
            assert row == [0] * FR.NSTAT
            continue
        assert set(counts) == screen_ref.set_ints(text, k), name
        assert row[FR.WINDOWS] == screen_ref.windows_ints(text, k) == row[FR.TAKEN], name
        assert row[FR.BASES] == fasta_ref.bases(text) == fasta_ref.brute_stretches(text)[1], name
        assert row[FR.RECORDS] == len(fasta_ref.records(text)), name


def test_what_the_cases_are_for():
    k = 21
    by = dict(FC.cases(k))
    row, _, counts = FR.spectrum_strings(by["poly_a_500"], k)
    assert counts == {0: 500 - k + 1} and row[FR.HIST_AT + 255] == 1
    assert FR.spectrum_strings(by["poly_a_500_unwrapped"], k)[2] == counts
    assert len(FR.spectrum_strings(by["dinucleotide"], k)[2]) == 2 and len(FR.spectrum_strings(by["tandem_7"], k)[2]) == 7
    row = FR.spectrum_strings(by["k_minus_1_and_k"], k)[0]
    assert row[FR.WINDOWS] == 1 and row[FR.RECORDS] == 3
    row, _, counts = FR.spectrum_strings(by["record_and_revcomp"], k)
    assert set(counts.values()) == {2} and row[FR.DISTINCT] == 250 - k + 1
    row, _, counts = FR.spectrum_strings(dict(FC.cases(16))["palindrome_16"], 16)
    assert max(counts.values()) == 2   # (the palindrome: once alone, once inside the second record; fw == rc)
    assert FR.spectrum_strings(by["n_every_%d" % (k - 1)], k)[0][FR.WINDOWS] == 0
    assert FR.spectrum_strings(by["n_every_%d" % k], k)[0][FR.WINDOWS] > 0
    assert FR.spectrum_strings(by["lower_case"], k)[2] == FR.spectrum_strings(by["lower_case"].upper(), k)[2]
    assert FR.spectrum_strings(by["header_only"], k)[0][:5] == [1, 0, 0, 0, 0]
    assert FR.spectrum_strings(b"", k) == ([0] * FR.NSTAT, 0, {})
    assert FR.spectrum_strings(by["two_headers_in_a_row"], k)[0][FR.RECORDS] == 3
    # a table too small: the status and a zero row
    assert FR.spectrum_strings(by["width_60"], k, slots=100)[:2] == ([0] * FR.NSTAT, FR.VK_SPEC_TABLE_FULL)
    assert FR.slots_for(0) == 1024 and FR.slots_for(513) == 2048 and FR.slots_for(4096, 4) == 2048


def test_assembly_estimate_and_report():
    k = 21
    text = dict(FC.cases(k))["record_and_revcomp"] + b">tail\n" + b"ACGTTGCATGCCATGACGTAGCTAGCTAAT\n"
    for every in (1, 4):
        row = FR.spectrum_numpy(text, k, every)[0]
        est = spectrum.assembly_estimate(row, k, every)
        assert est == FR.assembly_estimate(row, k, every)
        taken, distinct, ones = int(row[FR.TAKEN]), int(row[FR.DISTINCT]), int(row[FR.HIST_AT])
        assert est["genome_kmers"] == every * distinct and est["seen_fraction"] == 1.0 and est["reason"] == "assembly"
        assert est["high_copy_fraction"] == (taken - ones) / taken and est["singleton_fraction"] == ones / distinct
        assert all(est[x] is None for x in ("kmer_coverage", "base_coverage", "error_kmers", "error_rate"))
        rep = spectrum.report(row, k, every, assembly=True)
        reads = spectrum.report(row, k, every)
        assert rep["source"] == "assembly" and rep["records"] == 3 and "reads" not in rep and rep["estimates"] == est
        assert "source" not in reads and "records" not in reads and "seen_fraction" not in reads["estimates"]
        for key in ("k", "every", "bases", "windows", "taken_windows", "distinct", "histogram", "histogram_256_and_more"):
            assert rep[key] == reads[key]
        json.dumps(rep)
        cols = spectrum.assembly_columns(row, k, every)
        assert set(cols) == set(spectrum.columns(row, k, every))
        assert cols["spectrum_genome_kmers"] == every * distinct and cols["spectrum_high_copy_fraction"] == est["high_copy_fraction"]
        assert cols["spectrum_kmer_coverage"] == cols["spectrum_base_coverage"] == cols["spectrum_error_rate"] == ""
    empty = spectrum.assembly_estimate(np.zeros(FR.NSTAT, dtype=np.uint64), k)
    assert empty["genome_kmers"] == 0 and empty["high_copy_fraction"] is None and empty["singleton_fraction"] is None


def test_the_per_sample_form_agrees_with_the_old_one_on_reads():
    rng = random.Random(5)
    for _ in range(200):
        j = rng.choice([None, 0.0, 1.0, rng.random()])
        k, every, m = rng.choice([16, 21, 31]), rng.choice([1, 4]), rng.choice([1, 2, 3])
        est = [rng.choice([None, {"kmer_coverage": None, "genome_kmers": None},
                           {"kmer_coverage": rng.uniform(0.2, 30), "genome_kmers": rng.uniform(100, 1e6)}]) for _ in range(2)]
        a1, a2 = rng.randrange(1, 10 ** 6), rng.randrange(1, 10 ** 6)
        (eta1, g1), (eta2, g2) = sketch.sample_eta(est[0], m), sketch.sample_eta(est[1], m)
        assert sketch.corrected_distance(j, k, every, m, a1, est[0], a2, est[1]) == \
            sketch.corrected_distance_eta(j, k, every, a1, g1, eta1, a2, g2, eta2)
    # an assembly states its eta; two assemblies reduce to the Mash distance's exact form
    asm = {"kmer_coverage": None, "genome_kmers": 1000, "seen_fraction": 1.0}
    assert sketch.sample_eta(asm, 7) == (1.0, 1000)
    for j in (0.05, 1 / 3, 0.9, 1.0):
        # (two assemblies of a and b distinct k-mers: G = a, b; eligible = a, b)
        d = sketch.corrected_distance_eta(j, 21, 1, 1000, 1000, 1.0, 700, 700, 1.0)
        assert d == pytest.approx(1 - (2 * j / (1 + j)) ** (1 / 21), abs=1e-12)
        d4 = sketch.corrected_distance_eta(j, 21, 4, 250, 1000, 1.0, 175, 700, 1.0)
        assert d4 == pytest.approx(d, abs=1e-12)


def test_the_folder_check_exempts_assemblies_from_min_count(tmp_path):
    rng = random.Random(3)
    pool = sorted(rng.getrandbits(64) for _ in range(200))
    est = {"kmer_coverage": 2.0, "genome_kmers": 150.0}

    def put(folder, name, hashes, m, assembly):
        row = np.zeros(SR.NSTAT, dtype=np.uint64)
        row[SR.TAKEN] = row[SR.DISTINCT] = row[SR.HIST_AT] = len(hashes) + 3
        rep = spectrum.report(row, 21, 1, sketch=sketch.meta(64, m, len(hashes) + 3, len(hashes)), assembly=assembly)
        if not assembly:
            rep["estimates"].update(est)
        spectrum.write_report(folder, name, rep)
        sketch.write_sketch(folder, name, hashes)

    d = tmp_path / "D"
    put(d, "asm", pool[0:64], 1, True)
    put(d, "reads2", pool[32:96], 2, False)
    put(d, "reads2b", pool[10:74], 2, False)
    df = distance.run_distance(TSR.args_of(d, tmp_path / "OUT"), pairs=TSR.ref_pairs)
    assert list(df.columns) == distance.COLUMNS
    row = df[(df["sample"] == "reads2") & (df["neighbour"] == "asm")].iloc[0]
    jac = row["shared"] / row["seen"]
    want = sketch.corrected_distance_eta(jac, 21, 1, 67, 150.0, sketch.seen_fraction(2.0, 2), 67, 67, 1.0)
    assert row["corrected_distance"] == want
    # reads of another min_count are still refused, and named
    put(d, "reads3", pool[5:69], 3, False)
    with pytest.raises(Exception, match="min_count 2 and 3"):
        distance.run_distance(TSR.args_of(d, tmp_path / "OUT2"), pairs=TSR.ref_pairs)
    # an assembly of another size is refused like any other sample
    (d / "reads3.spectrum.json").unlink()
    row0 = np.zeros(SR.NSTAT, dtype=np.uint64)
    spectrum.write_report(d, "asm128", spectrum.report(row0, 21, 1, sketch=sketch.meta(128, 1, 0, 0), assembly=True))
    sketch.write_sketch(d, "asm128", [])
    with pytest.raises(Exception, match="size 64 and 128"):
        distance.run_distance(TSR.args_of(d, tmp_path / "OUT3"), pairs=TSR.ref_pairs)


# ------------------------------------------- an assembly against simulated libraries --

K, S, GENOME = TSR.K, TSR.S, TSR.GENOME
DIVERGENCES, DEPTHS, SEEDS = (0.01, 0.05), (1, 2, 4), (1, 2, 3, 4, 5)
# the worst |corrected - d| over the cells below, measured on the reference rule with these seeds (INTEGRATION.md has the
# table), plus a quarter
BOUND = {0.01: 1.25 * 0.00205, 0.05: 1.25 * 0.00161}


def assembly(g):
    """(eta, G, sketch, eligible) of the genome g (codes 0..3) as an assembly: its table by the rule's second statement."""
    text = FC.fa([(b"contig", TSR.LETTERS[g].tobytes())], 60)
    uniq, mult = FR.table_numpy(text, K)
    row = FR.spectrum_numpy(text, K)[0]
    eta, big_g = sketch.sample_eta(spectrum.assembly_estimate(row, K, 1), 1)
    sk, eligible = R.sketch_np(uniq, mult, 1, S)
    return eta, big_g, sk, eligible


@functools.lru_cache(maxsize=None)
def cells():
    """[(d, depth, seed, mash, corrected)]: computed once."""
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(2000 + seed)
        g1 = rng.integers(0, 4, GENOME, dtype=np.uint8)
        eta1, big_g1, sk1, el1 = assembly(g1)
        assert eta1 == 1.0 and big_g1 == el1
        for d in DIVERGENCES:
            g2 = g1.copy()
            sub = rng.random(GENOME) < d
            g2[sub] = (g2[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
            for depth in DEPTHS:
                est, sk2, el2 = TSR.library(TSR.reads_of(rng, g2, depth))
                eta2, big_g2 = sketch.sample_eta(est, 1)
                jac = sketch.jaccard(*R.pair_np(sk1, sk2, S))
                out.append((d, depth, seed, sketch.mash_distance(jac, K),
                            sketch.corrected_distance_eta(jac, K, 1, el1, big_g1, eta1, el2, big_g2, eta2)))
    return out


def test_the_corrected_distance_of_an_assembly_and_simulated_libraries():
    got = cells()
    assert len(got) == 30
    for d, depth, seed, mash, corr in got:
        print("d %.2f  depth %dx  seed %d  mash %.5f  corrected %.5f  error %+.5f" % (d, depth, seed, mash, corr, corr - d))
    for d in DIVERGENCES:
        print("worst |corrected - d| at d %.2f: %.5f" % (d, max(abs(c[4] - d) for c in got if c[0] == d)))
    for d, depth, seed, mash, corr in got:
        assert corr is not None and abs(corr - d) < abs(mash - d), (d, depth, seed)
        assert abs(corr - d) <= BOUND[d], (d, depth, seed, corr)
