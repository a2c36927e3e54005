"""`--genome-spectrum` end to end.  `image --from-fasta` on a plain and a .gz file with and without the flag: the PNG
pixels are equal, stats.csv differs only by the spectrum columns, `DIR/<sample>.spectrum.json`, `DIR/<sample>.sketch.npy`
and the two filled columns are the rule's (tests/fasta_spectrum_ref.py).  The same through `query --from-fasta`: the
predictions are those of a run without the flag.  `distance` over a folder that mixes reports of reads and of assemblies:
distances.csv is the host formula applied to the device's integers.  Every refusal exits with 2, names the flag and
writes nothing (no GPU needed for those)."""
import gzip
import json
import math

import numpy as np
import pytest

import fasta_spectrum_ref as FR
import sketch_ref as R
import spectrum_cases as SC
from screen_cases import fa, fq
from test_gpu_query_raw import model_files, query
from test_gpu_write_splits import pngs, run, same_images
from varkoder_amd import sketch as K
from varkoder_amd import spectrum as S

gpu = pytest.mark.gpu

NEW = ["spectrum_kmer_coverage", "spectrum_base_coverage", "spectrum_genome_kmers", "spectrum_error_rate",
       "spectrum_high_copy_fraction"]
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def genomes():
    """plain: two contigs, the second a copy of part of the first (copy number 2); zipped: one contig with N runs."""
    rng = np.random.default_rng(21)
    a = LETTERS[rng.integers(0, 4, 30000)].tobytes()
    b = LETTERS[rng.integers(0, 4, 20000)].tobytes()
    return {"plain": fa([(b"c1 first", a), (b"c2", a[5000:9000] + b[:3000])], 60),
            "zipped": fa([(b"z", b[:8000] + b"NNNNNNNNNN" + b[8000:])], 70)}


def write_genomes(folder):
    folder.mkdir(parents=True)
    texts = genomes()
    (folder / "plain.fasta").write_bytes(texts["plain"])
    (folder / "zipped.fa.gz").write_bytes(gzip.compress(texts["zipped"], compresslevel=1))
    return texts


def read_stats(path):
    import pandas as pd
    return pd.read_csv(path, float_precision="round_trip").set_index("sample")


def check_files(folder, sample, text, k, every, size):
    """the json and the .npy hold the rule's row and sketch of `text`"""
    row, status, keys, counts = FR.spectrum_numpy(text, k, every)
    assert status == 0 and int(row[FR.WINDOWS]) > 0
    h, eligible = R.sketch_np(keys, counts, 1, size)
    got = json.loads((folder / f"{sample}.spectrum.json").read_text())
    want = S.report(row, k, every, sketch=K.meta(size, 1, eligible, len(h)), assembly=True)
    assert got == json.loads(json.dumps(want)), sample
    assert got["source"] == "assembly" and got["records"] == int(row[FR.RECORDS]) and "reads" not in got
    assert got["estimates"] == json.loads(json.dumps(FR.assembly_estimate(row, k, every)))
    assert got["sketch"]["min_count"] == 1 and got["sketch"]["length"] == len(h)
    saved = np.load(folder / f"{sample}.sketch.npy")
    assert saved.dtype == np.uint64 and np.array_equal(saved, h)
    return row


@gpu
def test_image_from_fasta_with_and_without_the_flag(tmp_path):
    import pandas as pd
    texts = write_genomes(tmp_path / "asm")
    run(["asm", "--from-fasta", "-k", "7", "-o", "img0", "-f", "s0.csv"], tmp_path)
    run(["asm", "--from-fasta", "-k", "7", "-o", "img1", "-f", "s1.csv", "--genome-spectrum", "refs", "--spectrum-sketch", "64"], tmp_path)
    names = same_images(tmp_path / "img0", tmp_path / "img1")
    assert {n.split("@")[0] for n in names} == set(texts)
    a, b = pngs(tmp_path / "img0"), pngs(tmp_path / "img1")
    for name in a:
        assert a[name].read_bytes() == b[name].read_bytes(), name
    s0, s1 = read_stats(tmp_path / "s0.csv"), read_stats(tmp_path / "s1.csv")
    assert [c for c in s1.columns if c not in NEW] == list(s0.columns) and [c for c in s1.columns if c in NEW] == NEW
    keep = [c for c in s0.columns if not c.endswith("_time")]
    pd.testing.assert_frame_equal(s0[keep], s1[keep], check_exact=True)
    assert sorted(p.name for p in (tmp_path / "refs").iterdir()) == ["plain.sketch.npy", "plain.spectrum.json", "zipped.sketch.npy",
                                                                     "zipped.spectrum.json"]
    for s, t in texts.items():
        row = check_files(tmp_path / "refs", s, t, 21, 1, 64)
        est = FR.assembly_estimate(row, 21, 1)
        assert float(s1.loc[s, "spectrum_genome_kmers"]) == est["genome_kmers"]
        assert float(s1.loc[s, "spectrum_high_copy_fraction"]) == est["high_copy_fraction"]
        assert all(math.isnan(s1.loc[s, c]) for c in ("spectrum_kmer_coverage", "spectrum_base_coverage", "spectrum_error_rate"))
    assert json.loads((tmp_path / "refs" / "plain.spectrum.json").read_text())["estimates"]["high_copy_fraction"] > 0.1
    # other k and every, no sketch: no .npy, no "sketch" object
    run(["asm", "--from-fasta", "-k", "7", "-o", "img2", "-f", "s2.csv", "--genome-spectrum", "refs2", "--spectrum-k", "16",
         "--spectrum-every", "4"], tmp_path)
    assert sorted(p.name for p in (tmp_path / "refs2").iterdir()) == ["plain.spectrum.json", "zipped.spectrum.json"]
    for s, t in texts.items():
        row = FR.spectrum_numpy(t, 16, 4)[0]
        got = json.loads((tmp_path / "refs2" / f"{s}.spectrum.json").read_text())
        assert got == json.loads(json.dumps(S.report(row, 16, 4, assembly=True))) and "sketch" not in got


@gpu
def test_query_from_fasta_gives_the_same_predictions(tmp_path):
    texts = write_genomes(tmp_path / "asm")
    model_files(tmp_path)
    common = ["--from-fasta", "-b", "2", "-P"]
    query(tmp_path, tmp_path / "asm", tmp_path / "out0", *common)
    query(tmp_path, tmp_path / "asm", tmp_path / "out1", "--genome-spectrum", tmp_path / "refs", "--spectrum-sketch", "128", *common)
    a, b = ((tmp_path / d / "predictions.csv").read_text().replace(str(tmp_path / d), "") for d in ("out0", "out1"))
    assert a == b and a.count("\n") == 3
    for s, t in texts.items():
        check_files(tmp_path / "refs", s, t, 21, 1, 128)


@gpu
def test_distance_over_reads_and_assemblies(tmp_path):
    import pandas as pd
    from varkoder_amd import cli
    # an assembly, a diverged copy of it as a second assembly, and reads of the first at 20x with min_count 2
    rng = np.random.default_rng(31)
    g1 = rng.integers(0, 4, 20000, dtype=np.uint8)
    g2 = g1.copy()
    sub = rng.random(len(g2)) < 0.02
    g2[sub] = (g2[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
    (tmp_path / "asm").mkdir()
    (tmp_path / "asm" / "one.fa").write_bytes(fa([(b"g1", LETTERS[g1].tobytes())], 60))
    (tmp_path / "asm" / "two.fa").write_bytes(fa([(b"g2", LETTERS[g2].tobytes())], 80))
    reads = []
    for at in rng.integers(0, len(g1) - 100, 4000):
        reads.append(LETTERS[g1[at:at + 100]].tobytes())
    (tmp_path / "int" / "clean_reads").mkdir(parents=True)
    (tmp_path / "int" / "clean_reads" / "skim.fq.gz").write_bytes(gzip.compress(fq(reads), compresslevel=1))
    run(["asm", "--from-fasta", "-k", "7", "-o", "img_a", "-f", "sa.csv", "--genome-spectrum", "spec", "--spectrum-sketch", "1024"], tmp_path)
    run(["--from-clean", "int", "-k", "7", "-o", "img_r", "-f", "sr.csv", "-R", "7", "-m", "5K", "-M", "20K", "--kmer-spectrum", "spec",
         "--spectrum-sketch", "1024", "--spectrum-sketch-min-count", "2"], tmp_path)
    cli.main(["distance", str(tmp_path / "spec"), str(tmp_path / "out")])
    df = pd.read_csv(tmp_path / "out" / "distances.csv", float_precision="round_trip")
    reps = {s: json.loads((tmp_path / "spec" / f"{s}.spectrum.json").read_text()) for s in ("one", "two", "skim")}
    assert reps["one"]["source"] == reps["two"]["source"] == "assembly" and "source" not in reps["skim"]
    assert reps["skim"]["sketch"]["min_count"] == 2 and reps["skim"]["estimates"]["kmer_coverage"] is not None
    sk = {s: np.load(tmp_path / "spec" / f"{s}.sketch.npy") for s in reps}
    assert len(df) == 6
    for _, r in df.iterrows():
        a, b = reps[r["sample"]], reps[r["neighbour"]]
        shared, seen = R.pair_np(sk[r["sample"]], sk[r["neighbour"]], 1024)
        assert (int(r["shared"]), int(r["seen"])) == (shared, seen)
        jac = shared / seen
        eta1, big1 = K.sample_eta(a["estimates"], a["sketch"]["min_count"])
        eta2, big2 = K.sample_eta(b["estimates"], b["sketch"]["min_count"])
        want = K.corrected_distance_eta(jac, 21, 1, a["sketch"]["eligible"], big1, eta1, b["sketch"]["eligible"], big2, eta2)
        assert float(r["corrected_distance"]) == want and float(r["mash_distance"]) == K.mash_distance(jac, 21)
    by = {(r["sample"], r["neighbour"]): float(r["corrected_distance"]) for _, r in df.iterrows()}
    # assembly against assembly: the Mash distance's exact form; the skim is nearest to the genome it was read from
    jac = float(df[(df["sample"] == "one") & (df["neighbour"] == "two")]["jaccard"].iloc[0])
    assert by[("one", "two")] == pytest.approx(1 - (2 * jac / (1 + jac)) ** (1 / 21), abs=1e-12)
    assert by[("skim", "one")] < by[("skim", "two")] and by[("skim", "one")] < 0.005 and abs(by[("skim", "two")] - 0.02) < 0.01


def test_refusals(tmp_path, capsys, monkeypatch):
    """exit 2, before anything runs, naming the flag; nothing is written"""
    from varkoder_amd import cli
    monkeypatch.chdir(tmp_path)
    q = ["query", "-l", "m.pt", "--vocab", "v.txt", "in", "out"]
    bad = [
        (["image", "in", "--genome-spectrum", "d"], "--genome-spectrum"),                          # without --from-fasta
        (["image", "in", "--from-raw", "--genome-spectrum", "d"], "--genome-spectrum"),
        (["image", "in", "--from-clean", "--genome-spectrum", "d"], "--genome-spectrum"),
        (q + ["--genome-spectrum", "d"], "--genome-spectrum"),
        (q + ["--from-raw", "--genome-spectrum", "d"], "--genome-spectrum"),
        (q + ["--images", "--genome-spectrum", "d"], "--genome-spectrum"),
        (["image", "in", "--from-fasta", "--fragments", "--genome-spectrum", "d"], "--fragments"),
        (["image", "in", "--from-fasta", "--per-record", "--genome-spectrum", "d"], "--per-record"),
        (["image", "in", "--from-fasta", "--windows", "--genome-spectrum", "d"], "--windows"),
        (q + ["--from-fasta", "--per-record", "--genome-spectrum", "d"], "--per-record"),
        (q + ["--from-fasta", "--windows", "--genome-spectrum", "d"], "--windows"),
        (["image", "in", "--from-fasta", "--genome-spectrum", "d", "--spectrum-k", "15"], "--spectrum-k"),
        (q + ["--from-fasta", "--genome-spectrum", "d", "--spectrum-k", "32"], "--spectrum-k"),
        (["image", "in", "--from-fasta", "--genome-spectrum", "d", "--spectrum-every", "0"], "--spectrum-every"),
        (["image", "in", "--from-fasta", "--genome-spectrum", "d", "--spectrum-sketch", "63"], "--spectrum-sketch"),
        (["image", "in", "--from-fasta", "--genome-spectrum", "d", "--spectrum-sketch", "64", "--spectrum-sketch-min-count", "2"],
         "--spectrum-sketch-min-count"),
        (q + ["--from-fasta", "--genome-spectrum", "d", "--depth-filter", "2:10"], "--depth-filter"),
        (["image", "in", "--from-fasta", "--genome-spectrum", "d", "--kmer-spectrum", "e"], "-spectrum"),
        (["image", "in", "--from-fasta", "--spectrum-k", "21"], "--spectrum-k"),                  # without either
        (["image", "in", "--from-fasta", "--spectrum-sketch", "64"], "--spectrum-sketch"),
        (q + ["--from-fasta", "--spectrum-every", "4"], "--spectrum-every"),
    ]
    for argv, flag in bad:
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
        assert flag in capsys.readouterr().err.splitlines()[-1].split("error: ")[1], argv
    assert not list(tmp_path.iterdir())
    good = [
        (["image", "in", "--from-fasta", "--genome-spectrum", "d"], (21, 1, None)),
        (["image", "in", "--from-fasta", "--genome-spectrum", "d", "--spectrum-k", "16", "--spectrum-every", "16"], (16, 16, None)),
        (["image", "in", "--from-fasta", "--genome-spectrum", "d", "--spectrum-sketch", "16384"], (21, 1, 16384)),
        (q + ["--from-fasta", "--genome-spectrum", "d", "--spectrum-k", "31", "--spectrum-sketch", "64"], (31, 1, 64)),
    ]
    for argv, (k, every, size) in good:
        args = cli.parse_args(argv)
        g = cli.genome_spectrum_options(args)
        assert g is not None and (str(g.dir), g.k, g.every, g.sketch_size) == ("d", k, every, size)
        assert cli.spectrum_options(args) is None
    args = cli.parse_args(["image", "in", "--from-fasta"])
    assert cli.genome_spectrum_options(args) is None and not hasattr(args, "genome_spectrum")   # (opt-in: absent)
    # reads keep their flags
    sp = cli.spectrum_options(cli.parse_args(["image", "in", "--from-raw", "--kmer-spectrum", "d", "--spectrum-sketch", "64",
                                              "--spectrum-sketch-min-count", "2"]))
    assert (sp.sketch_size, sp.sketch_min_count) == (64, 2)
