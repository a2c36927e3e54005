"""`--kmer-spectrum` end to end.  `image --from-clean` on two tiny samples with and without the flag: the PNG files are
byte-identical, stats.csv differs only by the five columns, and `DIR/<sample>.spectrum.json` holds the histogram of
tests/spectrum_ref.py (one sample deep enough for estimates, one too shallow: empty cells).  The same through `image
--from-raw` with --exclude-fasta -- the spectrum is that of the screened text -- and through `query` (cleaned reads and
--from-raw).  Every refusal exits with 2, names the flag and writes nothing (no GPU needed for those)."""
import gzip
import json
import math

import numpy as np
import pytest

import clean_ref as C
import spectrum_cases as SC
import spectrum_ref as R
from screen_cases import fq
from test_gpu_query_raw import model_files, query
from test_gpu_write_splits import pngs, run
from varkoder_amd import spectrum as S

gpu = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "5K", "-M", "20K", "-k", "7"]
NEW = ["spectrum_kmer_coverage", "spectrum_base_coverage", "spectrum_genome_kmers", "spectrum_error_rate",
       "spectrum_high_copy_fraction"]
SETS = {"spA": C.synth_set(91, 500, 300), "spB": C.synth_set(92, 0, 1500)}


def clean_texts():
    """deep: 30x of a 20 kb genome in 100-base reads (estimates); shallow: 150 reads of a 2 Mb genome (none)."""
    rng = np.random.default_rng(11)
    return {"deep": fq(SC.simulated_reads(rng, 20000, 6000, 100, 0.005)),
            "shallow": fq(SC.simulated_reads(rng, 2000000, 150, 100, 0.005))}


def read_stats(path):
    import pandas as pd
    return pd.read_csv(path, float_precision="round_trip").set_index("sample")


def check_report(path, text, k, every):
    """the file holds the rule's row of `text` and the estimator's answer to it"""
    row, status = R.spectrum_numpy(text, k, every)
    assert status == 0 and int(row[R.READS]) > 0
    got = json.loads(path.read_text())
    assert got == json.loads(json.dumps(S.report(row, k, every))), path.name
    hist = [int(x) for x in row[R.HIST_AT:R.HIST_AT + 255]]
    assert got["histogram"] == hist[:len(got["histogram"])] and not any(hist[len(got["histogram"]):])
    assert (got["k"], got["every"], got["distinct"], got["histogram_256_and_more"]) == (k, every, int(row[R.DISTINCT]),
                                                                                     int(row[R.HIST_AT + 255]))
    return row


def check_columns(stats, sample, row, k, every):
    for name, v in S.columns(row, k, every).items():
        cell = stats.loc[sample, name]
        assert (isinstance(cell, float) and math.isnan(cell)) if v == "" else float(cell) == float(v), (sample, name)


@gpu
def test_image_from_clean_with_and_without_the_flag(tmp_path):
    import pandas as pd
    texts = clean_texts()
    (tmp_path / "int" / "clean_reads").mkdir(parents=True)
    for s, t in texts.items():
        (tmp_path / "int" / "clean_reads" / f"{s}.fq.gz").write_bytes(gzip.compress(t, compresslevel=1))
    run(["--from-clean", "int", "-o", "img0", "-f", "s0.csv"] + COMMON, tmp_path)
    run(["--from-clean", "int", "-o", "img1", "-f", "s1.csv", "--kmer-spectrum", "spec"] + COMMON, tmp_path)
    a, b = pngs(tmp_path / "img0"), pngs(tmp_path / "img1")
    assert a and sorted(a) == sorted(b) and {n.split("@")[0] for n in a} == set(texts)
    for name in a:
        assert a[name].read_bytes() == b[name].read_bytes(), name
    s0, s1 = read_stats(tmp_path / "s0.csv"), read_stats(tmp_path / "s1.csv")
    assert [c for c in s1.columns if c not in NEW] == list(s0.columns) and [c for c in s1.columns if c in NEW] == NEW
    keep = [c for c in s0.columns if not c.endswith("_time")]
    pd.testing.assert_frame_equal(s0[keep], s1[keep], check_exact=True)
    assert sorted(p.name for p in (tmp_path / "spec").iterdir()) == ["deep.spectrum.json", "shallow.spectrum.json"]
    assert not list(tmp_path.rglob("img0/**/*.spectrum.json")) and not [p for p in tmp_path.glob("*.spectrum.json")]
    rows = {s: check_report(tmp_path / "spec" / f"{s}.spectrum.json", t, 21, 1) for s, t in texts.items()}
    for s, row in rows.items():
        check_columns(s1, s, row, 21, 1)
    deep, shallow = (json.loads((tmp_path / "spec" / f"{s}.spectrum.json").read_text())["estimates"] for s in ("deep", "shallow"))
    assert deep["reason"] is None and deep["support"] >= 1000 and deep["genome_kmers"] > 0
    assert shallow["reason"] == "too few repeated k-mers" and shallow["kmer_coverage"] is None
    assert all(math.isnan(s1.loc["shallow", c]) for c in NEW) and not any(math.isnan(s1.loc["deep", c]) for c in NEW)


def write_raw(root, nested):
    for s, (r1, r2, se) in SETS.items():
        d = root / "tax" / s if nested else root / s
        d.mkdir(parents=True)
        if r1:
            (d / "lib_1.fq.gz").write_bytes(gzip.compress(C.fq(r1)))
            (d / "lib_2.fq.gz").write_bytes(gzip.compress(C.fq(r2)))
        if se:
            (d / "single.fastq").write_bytes(C.fq(se))


@gpu
def test_image_from_raw_counts_the_screened_text(tmp_path):
    write_raw(tmp_path / "raw", nested=True)
    ref = bytearray()   # every tenth read of both samples
    for s, (r1, _, se) in SETS.items():
        for i, (_, seq, _) in enumerate((r1 or se)[::10]):
            ref += b">%s_%d\n" % (s.encode(), i) + seq + b"\n"
    (tmp_path / "ref.fa").write_bytes(bytes(ref))
    run(["--from-raw", "raw", "-i", "int", "-o", "img", "-f", "s.csv", "--exclude-fasta", "ref.fa", "--screen-k", "25",
         "--kmer-spectrum", "spec", "--spectrum-k", "16", "--spectrum-every", "2"] + COMMON, tmp_path)
    stats = read_stats(tmp_path / "s.csv")
    for s in SETS:
        kept = gzip.decompress((tmp_path / "int" / "clean_reads" / f"{s}.fq.gz").read_bytes())   # (the screened text)
        row = check_report(tmp_path / "spec" / f"{s}.spectrum.json", kept, 16, 2)
        assert int(stats.loc[s, "screen_reads_removed"]) > 0
        assert int(row[R.READS]) == int(stats.loc[s, "screen_reads_in"]) - int(stats.loc[s, "screen_reads_removed"])
        check_columns(stats, s, row, 16, 2)
    # the same raw reads without the screen: more reads in the spectrum
    run(["--from-raw", "raw", "-o", "img2", "-f", "s2.csv", "--kmer-spectrum", "spec2", "--spectrum-k", "16",
         "--spectrum-every", "2"] + COMMON, tmp_path)
    for s in SETS:
        a, b = (json.loads((tmp_path / d / f"{s}.spectrum.json").read_text()) for d in ("spec", "spec2"))
        assert b["reads"] == int(stats.loc[s, "screen_reads_in"]) > a["reads"]


@gpu
def test_query_writes_the_spectra(tmp_path):
    write_raw(tmp_path / "rawq", nested=False)
    model_files(tmp_path)
    common = ["-R", "5", "-M", "20K", "-b", "2", "-P"]
    query(tmp_path, tmp_path / "rawq", tmp_path / "out1", "--from-raw", "-i", tmp_path / "intq", "--kmer-spectrum", tmp_path / "spec1",
          *common)
    clean = {s: gzip.decompress((tmp_path / "intq" / "clean_reads" / f"{s}.fq.gz").read_bytes()) for s in SETS}
    for s, text in clean.items():
        check_report(tmp_path / "spec1" / f"{s}.spectrum.json", text, 21, 1)
    # the cleaned reads of that run, as query's default entry takes them
    query(tmp_path, tmp_path / "intq" / "clean_reads", tmp_path / "out2", "--kmer-spectrum", tmp_path / "spec2", "--spectrum-k", "31",
          *common)
    for s, text in clean.items():
        check_report(tmp_path / "spec2" / f"{s}.spectrum.json", text, 31, 1)
    query(tmp_path, tmp_path / "intq" / "clean_reads", tmp_path / "out3", *common)
    a, b = ((tmp_path / d / "predictions.csv").read_text().replace(str(tmp_path / d), "") for d in ("out2", "out3"))
    assert a == b and a.count("\n") == 3   # (without the flag: the same predictions)


def test_refusals(tmp_path, capsys, monkeypatch):
    """exit 2, before anything runs, naming the flag; nothing is written"""
    from varkoder_amd import cli
    monkeypatch.chdir(tmp_path)
    q = ["query", "-l", "m.pt", "--vocab", "v.txt", "in", "out"]
    bad = [
        (["image", "in", "--kmer-spectrum", "d"], "--kmer-spectrum"),                             # the default entry (step D)
        (["image", "in", "--from-fasta", "--kmer-spectrum", "d"], "--kmer-spectrum"),
        (q + ["--from-fasta", "--kmer-spectrum", "d"], "--kmer-spectrum"),
        (q + ["--images", "--kmer-spectrum", "d"], "--kmer-spectrum"),
        (["image", "in", "--from-raw", "--kmer-spectrum", "d", "--spectrum-k", "15"], "--spectrum-k"),
        (["image", "in", "--from-clean", "--kmer-spectrum", "d", "--spectrum-k", "32"], "--spectrum-k"),
        (q + ["--kmer-spectrum", "d", "--spectrum-k", "0"], "--spectrum-k"),
        (["image", "in", "--from-bam", "--kmer-spectrum", "d", "--spectrum-every", "0"], "--spectrum-every"),
        (q + ["--from-raw", "--kmer-spectrum", "d", "--spectrum-every", "-4"], "--spectrum-every"),
        (["image", "in", "--from-raw", "--spectrum-k", "21"], "--spectrum-k"),                    # without --kmer-spectrum
        (["image", "in", "--from-clean", "--spectrum-every", "16"], "--spectrum-every"),
        (q + ["--spectrum-k", "21"], "--spectrum-k"),
        (q + ["--from-raw", "--spectrum-every", "2"], "--spectrum-every"),
    ]
    for argv, flag in bad:
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
        assert flag in capsys.readouterr().err.splitlines()[-1].split("error: ")[1], argv
    assert not list(tmp_path.iterdir())
    good = [
        (["image", "in", "--from-raw", "--kmer-spectrum", "d"], (21, 1)),
        (["image", "in", "--from-clean", "--kmer-spectrum", "d", "--spectrum-k", "16", "--spectrum-every", "16"], (16, 16)),
        (["image", "in", "--from-bam", "--bam-pairs", "--kmer-spectrum", "d", "--spectrum-k", "31"], (31, 1)),
        (q + ["--kmer-spectrum", "d", "--spectrum-every", "4"], (21, 4)),
        (q + ["--from-raw", "--kmer-spectrum", "d"], (21, 1)),
        (q + ["--from-bam", "--kmer-spectrum", "d"], (21, 1)),
    ]
    for argv, (k, every) in good:
        sp = cli.spectrum_options(cli.parse_args(argv))
        assert sp is not None and (str(sp.dir), sp.k, sp.every) == ("d", k, every)
    args = cli.parse_args(["image", "in", "--from-raw"])
    assert cli.spectrum_options(args) is None
    assert not [n for n in ("kmer_spectrum", "spectrum_k", "spectrum_every") if hasattr(args, n)]   # (opt-in: absent)
