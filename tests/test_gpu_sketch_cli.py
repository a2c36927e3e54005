"""`--spectrum-sketch` and `distance` end to end.  `image --from-clean --kmer-spectrum D --spectrum-sketch 256` on three
tiny samples: every `.sketch.npy` and `"sketch"` object is what tests/sketch_ref.py gives; `distance D OUT --matrix` writes
what sketch_ref and varkoder_amd/sketch.py give.  The same `image` run without the flag writes the reports and the stats
of the spectrum alone: no `sketch` key, no `.npy`, and the run with the flag differs from it by those alone.  `query`
accepts the flags.  Every refusal exits with 2 and names the flag (no GPU needed for those)."""
import gzip
import json

import numpy as np
import pytest

import sketch_ref as R
import spectrum_cases as SC
import spectrum_ref as SR
from screen_cases import fq
from test_gpu_query_raw import model_files, query
from test_gpu_spectrum_cli import read_stats
from test_gpu_write_splits import pngs, run
from varkoder_amd import cli, sketch
from varkoder_amd import spectrum as S

gpu = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "5K", "-M", "20K", "-k", "7"]
SIZE = 256


def clean_texts():
    """two libraries of one 20 kb genome at 30x and 1x, and one of another genome"""
    rng = np.random.default_rng(12)
    g = rng.integers(0, 4, 20000, dtype=np.uint8)

    def reads(genome, n):
        at = rng.integers(0, len(genome) - 100 + 1, n)
        r = genome[at[:, None] + np.arange(100)[None, :]]
        return [x.tobytes() for x in np.frombuffer(b"ACGT", dtype=np.uint8)[r]]
    return {"deep": fq(reads(g, 6000)), "same": fq(reads(g, 200)), "other": fq(SC.simulated_reads(rng, 20000, 3000, 100, 0.005))}


def want_sketch(text, k, m, s):
    counts = SR.counts_loop(text, k, 1)[3]
    return R.sketch_np(list(counts.keys()), list(counts.values()), m, s)


@gpu
def test_image_with_the_flag_then_distance_and_without_it(tmp_path):
    import pandas as pd
    texts = clean_texts()
    (tmp_path / "int" / "clean_reads").mkdir(parents=True)
    for s, t in texts.items():
        (tmp_path / "int" / "clean_reads" / f"{s}.fq.gz").write_bytes(gzip.compress(t, compresslevel=1))
    run(["--from-clean", "int", "-o", "img0", "-f", "s0.csv", "--kmer-spectrum", "D0"] + COMMON, tmp_path)
    run(["--from-clean", "int", "-o", "img1", "-f", "s1.csv", "--kmer-spectrum", "D", "--spectrum-sketch", str(SIZE)] + COMMON, tmp_path)
    names = sorted(texts)
    # without the flag: the reports alone, no sketch key; with it the same reports plus the key, the same stats and images
    assert sorted(p.name for p in (tmp_path / "D0").iterdir()) == [f"{s}.spectrum.json" for s in names]
    assert sorted(p.name for p in (tmp_path / "D").iterdir()) == sorted([f"{s}.spectrum.json" for s in names] +
                                                                        [f"{s}.sketch.npy" for s in names])
    sketches = {}
    for s in names:
        plain = (tmp_path / "D0" / f"{s}.spectrum.json").read_text()
        row, status = SR.spectrum_numpy(texts[s], 21, 1)
        assert status == 0 and plain == json.dumps(S.report(row, 21, 1)) and "sketch" not in json.loads(plain)
        got = json.loads((tmp_path / "D" / f"{s}.spectrum.json").read_text())
        sk, eligible = want_sketch(texts[s], 21, 1, SIZE)
        assert got.pop("sketch") == {"size": SIZE, "min_count": 1, "eligible": eligible, "length": SIZE,
                                     "hash": "splitmix64-finaliser", "version": 1}
        assert json.dumps(got) == plain
        npy = np.load(tmp_path / "D" / f"{s}.sketch.npy")
        assert npy.dtype == np.uint64 and np.array_equal(npy, sk) and eligible > SIZE
        sketches[s] = sk
    s0, s1 = read_stats(tmp_path / "s0.csv"), read_stats(tmp_path / "s1.csv")
    keep = [c for c in s0.columns if not c.endswith("_time")]
    assert list(s0.columns) == list(s1.columns)
    pd.testing.assert_frame_equal(s0[keep], s1[keep], check_exact=True)
    a, b = pngs(tmp_path / "img0"), pngs(tmp_path / "img1")
    assert a and sorted(a) == sorted(b) and all(a[n].read_bytes() == b[n].read_bytes() for n in a)
    # distance
    cli.main(["distance", str(tmp_path / "D"), str(tmp_path / "OUT"), "--matrix"])
    shared, seen = np.load(tmp_path / "OUT" / "shared.npy"), np.load(tmp_path / "OUT" / "seen.npy")
    corr = np.load(tmp_path / "OUT" / "corrected_distance.npy")
    assert (tmp_path / "OUT" / "distances_rows.txt").read_text().split() == names
    assert (tmp_path / "OUT" / "distances_cols.txt").read_text().split() == names
    reports = {s: json.loads((tmp_path / "D" / f"{s}.spectrum.json").read_text()) for s in names}
    table = pd.read_csv(tmp_path / "OUT" / "distances.csv", float_precision="round_trip")
    assert list(table.columns) == ["sample", "neighbour", "rank", "shared", "seen", "jaccard", "mash_distance", "corrected_distance"]
    assert len(table) == 6
    for i, x in enumerate(names):
        for j, y in enumerate(names):
            want = R.pair_loop(sketches[x], sketches[y], SIZE)
            assert (int(shared[i, j]), int(seen[i, j])) == want, (x, y)
            jac = sketch.jaccard(*want)
            cd = sketch.corrected_distance(jac, 21, 1, 1, reports[x]["sketch"]["eligible"], reports[x]["estimates"],
                                           reports[y]["sketch"]["eligible"], reports[y]["estimates"])
            assert (cd is None and np.isnan(corr[i, j])) or corr[i, j] == cd
            if i != j:
                row = table[(table["sample"] == x) & (table["neighbour"] == y)].iloc[0]
                assert (row["shared"], row["seen"]) == want and row["jaccard"] == jac
                assert row["mash_distance"] == sketch.mash_distance(jac, 21)
                assert (cd is None and np.isnan(row["corrected_distance"])) or row["corrected_distance"] == cd
    deep = table[table["sample"] == "deep"]
    assert list(deep["neighbour"]) == ["same", "other"] and list(deep["rank"]) == [1, 2]
    # two libraries of one genome at 30x and 1x: the corrected distance says so, the raw Jaccard index does not
    first = deep.iloc[0]
    assert first["corrected_distance"] < 0.005 < first["mash_distance"]
    # an existing OUT is refused without -x
    with pytest.raises(Exception, match="exists"):
        cli.main(["distance", str(tmp_path / "D"), str(tmp_path / "OUT")])
    cli.main(["distance", str(tmp_path / "D"), str(tmp_path / "OUT"), "-x", "--against", str(tmp_path / "D"), "-N", "1"])
    again = pd.read_csv(tmp_path / "OUT" / "distances.csv")
    assert list(again["neighbour"]) == names and list(again["jaccard"]) == [1.0] * 3   # (nothing excluded: each its own nearest)


@gpu
def test_query_accepts_the_flags(tmp_path):
    texts = clean_texts()
    (tmp_path / "clean").mkdir()
    for s, t in texts.items():
        (tmp_path / "clean" / f"{s}.fq.gz").write_bytes(gzip.compress(t, compresslevel=1))
    model_files(tmp_path)
    query(tmp_path, tmp_path / "clean", tmp_path / "out", "--kmer-spectrum", tmp_path / "D", "--spectrum-k", "16",
          "--spectrum-sketch", "64", "--spectrum-sketch-min-count", "2", "-R", "5", "-M", "20K", "-b", "2", "-P")
    for s, t in texts.items():
        sk, eligible = want_sketch(t, 16, 2, 64)
        got = json.loads((tmp_path / "D" / f"{s}.spectrum.json").read_text())
        assert got["sketch"]["eligible"] == eligible and got["sketch"]["min_count"] == 2 and got["k"] == 16
        assert np.array_equal(np.load(tmp_path / "D" / f"{s}.sketch.npy"), sk)


def test_refusals(tmp_path, capsys, monkeypatch):
    """exit 2, before anything runs, naming the flag; nothing is written"""
    monkeypatch.chdir(tmp_path)
    q = ["query", "-l", "m.pt", "--vocab", "v.txt", "in", "out"]
    for argv, flag in (
            (["image", "in", "--from-clean", "--spectrum-sketch", "256"], "--spectrum-sketch"),                      # without --kmer-spectrum
            (q + ["--spectrum-sketch", "256"], "--spectrum-sketch"),
            (["image", "in", "--from-raw", "--spectrum-sketch-min-count", "2"], "--spectrum-sketch-min-count"),
            (["image", "in", "--from-clean", "--kmer-spectrum", "d", "--spectrum-sketch", "63"], "--spectrum-sketch"),
            (q + ["--kmer-spectrum", "d", "--spectrum-sketch", str((1 << 20) + 1)], "--spectrum-sketch"),
            (["image", "in", "--from-clean", "--kmer-spectrum", "d", "--spectrum-sketch-min-count", "2"], "--spectrum-sketch-min-count"),
            (["image", "in", "--from-bam", "--kmer-spectrum", "d", "--spectrum-sketch", "64", "--spectrum-sketch-min-count", "0"],
             "--spectrum-sketch-min-count"),
            (["distance", "d", "out", "-N", "0"], "-N")):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2 and flag in capsys.readouterr().err, argv
    assert not list(tmp_path.iterdir())
    for argv, want in ((["image", "in", "--from-raw", "--kmer-spectrum", "d", "--spectrum-sketch", "64"], (64, 1)),
                       (q + ["--kmer-spectrum", "d", "--spectrum-sketch", str(1 << 20), "--spectrum-sketch-min-count", "3"], (1 << 20, 3)),
                       (["image", "in", "--from-clean", "--kmer-spectrum", "d"], (None, 1))):
        opt = cli.spectrum_options(cli.parse_args(argv))
        assert (opt.sketch_size, opt.sketch_min_count) == want
