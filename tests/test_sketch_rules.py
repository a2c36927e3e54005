"""The rule of `--spectrum-sketch` and `distance` without a GPU: the two statements of tests/sketch_ref.py agree on every
case; the bottom-s comparison of two sketches equals that of the full sets; below s it is the exact Jaccard index; the
files of `distance` round-trip and every refusal fires; without the flag a report has no `sketch` key; and the corrected
distance, on simulated libraries of known divergence and unequal depth, is nearer the truth than the Mash distance in
every cell and within the bound measured on these seeds (the table: INTEGRATION.md, next to the rule)."""
import functools
import json
import random
import types

import numpy as np
import pytest

import sketch_cases as KC
import sketch_ref as R
import spectrum_ref as SR
from varkoder_amd import distance, sketch, spectrum


# ------------------------------------------------------------------ the rule --

def test_unmix_is_the_inverse_of_the_mix():
    rng = random.Random(1)
    assert (R.C1 * KC.INV1) % (1 << 64) == 1 and (R.C2 * KC.INV2) % (1 << 64) == 1
    for h in [0, 1, R.MASK - 1, 1 << 63] + [rng.getrandbits(64) for _ in range(200)]:
        assert R.mix(KC.unmix(h)) == h
    z = np.array([rng.getrandbits(64) for _ in range(100)], dtype=np.uint64)
    assert R.mix_np(z).tolist() == [R.mix(int(x)) for x in z]


def test_the_two_statements_agree_on_every_table():
    for t in KC.hand_tables() + [KC.big_table()]:
        loop, el = R.sketch_loop(t.keys, t.counts, t.m, t.s)
        vec, ev = R.sketch_np(t.keys, t.counts, t.m, t.s)
        assert loop == vec.tolist() and el == ev and len(loop) == min(t.s, el), t.name
        assert all(a < b for a, b in zip(loop, loop[1:])), t.name   # strictly ascending: the mix is a bijection
    with pytest.raises(ValueError):
        t = KC.duplicate_table()
        R.sketch_loop(t.keys, t.counts, t.m, t.s)


def test_the_two_statements_agree_on_every_pair():
    s = 64
    sketches = [x for _, a, b in KC.seam_pairs(s) for x in (a, b)]
    for a in sketches:
        for b in sketches:
            assert R.pair_loop(a, b, s) == R.pair_np(a, b, s)
    assert R.pair_loop([], [], s) == (0, 0)


def test_sketches_compare_as_the_full_sets_do():
    """the seen smallest of Sa u Sb are the s smallest of the full union, and one of them lies in both sketches exactly
    when it lies in both full sets"""
    rng = random.Random(7)
    for s, na, nb, common in ((64, 500, 300, 200), (64, 64, 64, 10), (100, 30, 5000, 20), (64, 70, 63, 63), (64, 10, 20, 5)):
        pool = KC.spread(rng, na + nb)
        both = pool[:common]
        ha, hb = set(both + pool[common:na]), set(both + pool[na:na + nb - common])
        got = R.pair_loop(R.bottom(ha, s), R.bottom(hb, s), s)
        assert got == R.full_pair(ha, hb, s), (s, na, nb)
        if len(ha) < s and len(hb) < s:   # below s: the exact Jaccard index of the full sets
            assert got == (len(ha & hb), len(ha | hb))


# --------------------------------------------------------- the files of `distance` --

def write_folder(folder, samples, k=21, every=1, size=64, m=1, **change):
    """A folder as `--kmer-spectrum DIR --spectrum-sketch S` writes it: samples = {name: (hashes, estimates or None)}."""
    for name, (hashes, est) in samples.items():
        row = np.zeros(SR.NSTAT, dtype=np.uint64)
        rep = spectrum.report(row, k, every, sketch=sketch.meta(size, m, len(hashes) + 3, len(hashes)))
        if est is not None:
            rep["estimates"].update(est)
        for key, v in change.get(name, {}).items():
            if key in rep["sketch"]:
                rep["sketch"][key] = v
            else:
                rep[key] = v
        spectrum.write_report(folder, name, rep)
        sketch.write_sketch(folder, name, hashes)


def ref_pairs(q, ql, r, rl, s):
    out = np.zeros((2, len(q), len(r)), dtype=np.uint32)
    for i in range(len(q)):
        for j in range(len(r)):
            out[:, i, j] = R.pair_loop(q[i, :int(ql[i])], r[j, :int(rl[j])], s)
    return out[0], out[1]


def args_of(inp, out, against=None, n=10, matrix=False, overwrite=False):
    return types.SimpleNamespace(input=str(inp), outdir=str(out), against=None if against is None else str(against), neighbours=n,
                                 matrix=matrix, overwrite=overwrite)


EST = {"kmer_coverage": 2.0, "genome_kmers": 150.0}


def folder_samples():
    rng = random.Random(3)
    pool = KC.spread(rng, 200)
    return {"a": (pool[0:64], EST), "b": (pool[32:96], EST), "c": (pool[0:64], None), "d": ([], EST), "e": (pool[100:130], EST)}


def test_distance_files_round_trip(tmp_path):
    samples = folder_samples()
    write_folder(tmp_path / "D", samples)
    (tmp_path / "D" / "plain.spectrum.json").write_text(json.dumps(spectrum.report(np.zeros(SR.NSTAT, dtype=np.uint64), 21)))
    df = distance.run_distance(args_of(tmp_path / "D", tmp_path / "OUT", matrix=True), pairs=ref_pairs)
    names = sorted(samples)
    assert list(df.columns) == distance.COLUMNS and sorted(set(df["sample"])) == names   # (the report without a sketch is no sample)
    import pandas as pd
    back = pd.read_csv(tmp_path / "OUT" / "distances.csv")
    shared, seen = np.load(tmp_path / "OUT" / "shared.npy"), np.load(tmp_path / "OUT" / "seen.npy")
    corr = np.load(tmp_path / "OUT" / "corrected_distance.npy")
    assert (tmp_path / "OUT" / "distances_rows.txt").read_text().split() == names
    assert (tmp_path / "OUT" / "distances_cols.txt").read_text().split() == names
    assert shared.dtype == np.uint32 and shared.shape == (5, 5) and corr.dtype == np.float64
    for i, a in enumerate(names):
        rows = back[back["sample"] == a]
        assert list(rows["rank"]) == [1, 2, 3, 4] and a not in set(rows["neighbour"])   # self is excluded
        jac = [-1.0 if se == 0 else sh / se for sh, se in zip(rows["shared"], rows["seen"])]
        idx = [names.index(x) for x in rows["neighbour"]]
        assert all((jac[n], -idx[n]) > (jac[n + 1], -idx[n + 1]) for n in range(3))     # jaccard descending, then the lower index
        for _, row in rows.iterrows():
            j = names.index(row["neighbour"])
            want = R.pair_loop(samples[a][0], samples[names[j]][0], 64)
            assert (row["shared"], row["seen"]) == want == (shared[i, j], seen[i, j])
            jv = sketch.jaccard(*want)
            assert (np.isnan(row["jaccard"]) and jv is None) or row["jaccard"] == pytest.approx(jv, rel=1e-12)
            cd = sketch.corrected_distance(jv, 21, 1, 1, len(samples[a][0]) + 3, samples[a][1], len(samples[names[j]][0]) + 3,
                                           samples[names[j]][1])
            assert (np.isnan(corr[i, j]) and cd is None) or corr[i, j] == cd
            assert (np.isnan(row["corrected_distance"]) and cd is None) or row["corrected_distance"] == pytest.approx(cd, rel=1e-12)
    assert np.isnan(corr[names.index("a"), names.index("c")])     # c has no estimates
    assert np.isnan(corr[names.index("d"), names.index("d")])     # nothing seen: no jaccard
    a_rows = back[back["sample"] == "a"]
    assert list(a_rows["neighbour"])[0] == "c" and list(a_rows["mash_distance"])[0] == 0.0
    # --against: nothing excluded, -N cuts
    df = distance.run_distance(args_of(tmp_path / "D", tmp_path / "OUT2", against=tmp_path / "D", n=2), pairs=ref_pairs)
    assert len(df) == 10 and list(df[df["sample"] == "a"]["neighbour"]) == ["a", "c"]
    assert not (tmp_path / "OUT2" / "shared.npy").exists()


def test_distance_refusals(tmp_path, monkeypatch):
    samples = folder_samples()
    write_folder(tmp_path / "D", samples)
    with pytest.raises(Exception, match="exists"):
        (tmp_path / "OUT").mkdir()
        distance.run_distance(args_of(tmp_path / "D", tmp_path / "OUT"), pairs=ref_pairs)
    distance.run_distance(args_of(tmp_path / "D", tmp_path / "OUT", overwrite=True), pairs=ref_pairs)
    with pytest.raises(Exception, match="does not exist"):
        distance.run_distance(args_of(tmp_path / "D", tmp_path / "O2", against=tmp_path / "nowhere"), pairs=ref_pairs)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(Exception, match="one GPU"):
        distance.run_distance(args_of(tmp_path / "D", tmp_path / "O3"), pairs=ref_pairs)
    monkeypatch.delenv("WORLD_SIZE")
    for n, (key, value) in enumerate((("k", 25), ("every", 4), ("size", 128), ("min_count", 2), ("hash", "other"), ("version", 2))):
        folder = tmp_path / ("X%d" % n)
        write_folder(folder, samples, b={key: value})
        with pytest.raises(Exception) as e:
            distance.run_distance(args_of(folder, tmp_path / ("XO%d" % n)), pairs=ref_pairs)
        msg = str(e.value)
        assert "a.spectrum.json" in msg and "b.spectrum.json" in msg and key in msg, msg
        # the same between SPECTRA and REF_SPECTRA
        write_folder(tmp_path / ("Y%d" % n), {"z": samples["a"]}, z={key: value})
        with pytest.raises(Exception) as e:
            distance.run_distance(args_of(tmp_path / "D", tmp_path / ("YO%d" % n), against=tmp_path / ("Y%d" % n)), pairs=ref_pairs)
        assert "a.spectrum.json" in str(e.value) and "z.spectrum.json" in str(e.value)
    write_folder(tmp_path / "V", samples, **{name: {"version": 2} for name in samples})
    with pytest.raises(Exception, match="version"):
        distance.run_distance(args_of(tmp_path / "V", tmp_path / "VO"), pairs=ref_pairs)
    (tmp_path / "E").mkdir()
    with pytest.raises(Exception, match="no .spectrum.json"):
        distance.run_distance(args_of(tmp_path / "E", tmp_path / "EO"), pairs=ref_pairs)
    np.save(sketch.sketch_path(tmp_path / "D", "a"), np.zeros(3, dtype=np.uint64))
    with pytest.raises(Exception, match="not the sketch"):
        distance.run_distance(args_of(tmp_path / "D", tmp_path / "DO"), pairs=ref_pairs)


def test_without_the_flag_a_report_has_no_sketch_key():
    row = np.arange(SR.NSTAT, dtype=np.uint64)
    plain = spectrum.report(row, 21, 1)
    assert "sketch" not in plain and list(plain) == ["k", "every", "reads", "bases", "windows", "taken_windows", "distinct",
                                                     "histogram", "histogram_256_and_more", "estimates"]
    with_sketch = spectrum.report(row, 21, 1, sketch=sketch.meta(256, 2, 1000, 256))
    assert with_sketch["sketch"] == {"size": 256, "min_count": 2, "eligible": 1000, "length": 256, "hash": "splitmix64-finaliser",
                                     "version": 1}
    del with_sketch["sketch"]
    assert json.dumps(with_sketch) == json.dumps(plain)
    from varkoder_amd.pipeline import Spectrum
    assert Spectrum("D").sketch_size is None and Spectrum("D").sketch_min_count == 1


def test_the_distances():
    assert sketch.jaccard(0, 0) is None and sketch.jaccard(3, 4) == 0.75
    assert sketch.mash_distance(None, 21) is None and sketch.mash_distance(0.0, 21) == 1.0 and sketch.mash_distance(1.0, 21) == 0.0
    assert sketch.seen_fraction(2.0, 1) == pytest.approx(1 - np.exp(-2.0)) and sketch.seen_fraction(2.0, 3) == pytest.approx(1 - 5 * np.exp(-2.0))
    est = {"kmer_coverage": 30.0, "genome_kmers": 1000.0}
    # deep, error-free, identical: J = 1, I = A -> D = 0; half the k-mers shared -> (1 - D)^k = 1 / 2
    assert sketch.corrected_distance(1.0, 21, 1, 1, 1000, est, 1000, est) == pytest.approx(0.0, abs=1e-12)
    assert sketch.corrected_distance(1 / 3, 21, 1, 1, 1000, est, 1000, est) == pytest.approx(1 - 0.5 ** (1 / 21))
    assert sketch.corrected_distance(1 / 3, 21, 4, 1, 250, est, 250, est) == pytest.approx(1 - 0.5 ** (1 / 21))   # every = 4
    assert sketch.corrected_distance(0.0, 21, 1, 1, 1000, est, 1000, est) == 1.0
    assert sketch.corrected_distance(None, 21, 1, 1, 0, est, 0, est) is None
    assert sketch.corrected_distance(0.5, 21, 1, 1, 10, {"kmer_coverage": None, "genome_kmers": None}, 10, est) is None


# ------------------------------------------------------- the estimator, simulated --

K, S, GENOME, LENGTH, ERROR = 21, 16384, 200000, 150, 0.005
DIVERGENCES, DEPTHS, SEEDS = (0.01, 0.05), ((1, 4), (2, 8)), (1, 2, 3, 4, 5)
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
# the worst |corrected - d| over the cells below, measured (INTEGRATION.md has the table), plus a quarter
BOUND = {0.01: 1.25 * 0.00188, 0.05: 1.25 * 0.00380}


def reads_of(rng, g, depth):
    """Reads of LENGTH bases from the genome g (codes 0..3), either strand, every base substituted with probability ERROR."""
    n = depth * len(g) // LENGTH
    at = rng.integers(0, len(g) - LENGTH + 1, n)
    r = g[at[:, None] + np.arange(LENGTH)[None, :]]
    flip = rng.random(n) < 0.5
    r[flip] = (3 - r[flip])[:, ::-1]
    err = rng.random(r.shape) < ERROR
    r[err] = (r[err] + rng.integers(1, 4, int(err.sum()), dtype=np.uint8)) & 3
    return [x.tobytes() for x in LETTERS[r]]


def library(seqs):
    """(estimates, sketch, eligible) of a library: its table by spectrum_ref's second statement."""
    keys = SR.keys_numpy(seqs, K)
    uniq, mult = np.unique(keys, return_counts=True)
    row = np.zeros(SR.NSTAT, dtype=np.uint64)
    row[SR.READS], row[SR.BASES], row[SR.WINDOWS] = len(seqs), sum(len(x) for x in seqs), len(keys)
    row[SR.TAKEN], row[SR.DISTINCT] = len(keys), len(uniq)
    row[SR.HIST_AT:] = np.bincount(np.minimum(mult, SR.BINS) - 1, minlength=SR.BINS)
    sk, eligible = R.sketch_np(uniq, mult, 1, S)
    return spectrum.estimate(row, K, 1), sk, eligible


@functools.lru_cache(maxsize=None)
def cells():
    """[(d, depths, seed, mash, corrected)]: computed once."""
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(1000 + seed)
        g1 = rng.integers(0, 4, GENOME, dtype=np.uint8)
        for d in DIVERGENCES:
            g2 = g1.copy()
            sub = rng.random(GENOME) < d
            g2[sub] = (g2[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
            for da, db in DEPTHS:
                ea, ska, ela = library(reads_of(rng, g1, da))
                eb, skb, elb = library(reads_of(rng, g2, db))
                jac = sketch.jaccard(*R.pair_np(ska, skb, S))
                out.append((d, (da, db), seed, sketch.mash_distance(jac, K),
                            sketch.corrected_distance(jac, K, 1, 1, ela, ea, elb, eb)))
    return out


def test_the_corrected_distance_on_simulated_libraries():
    got = cells()
    assert len(got) == 20
    for d, depths, seed, mash, corr in got:
        print("d %.2f  depths %dx %dx  seed %d  mash %.5f  corrected %.5f  error %+.5f" % (d, *depths, seed, mash, corr, corr - d))
    for d, depths, seed, mash, corr in got:
        assert corr is not None and abs(corr - d) < abs(mash - d), (d, depths, seed)
        assert abs(corr - d) <= BOUND[d], (d, depths, seed, corr)
