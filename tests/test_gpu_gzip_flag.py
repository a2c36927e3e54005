"""`--gpu-gzip` end to end: the same commands with and without the flag leave files of the same names whose text is the
same byte for byte, the same stats, images and predictions; the flag's files are BGZF that the product's own entries read."""
import gzip
from pathlib import Path

import pytest

import clean_ref as R
from test_gpu_query_raw import model_files, query
from test_gpu_write_splits import COMMON, run, same_images, sample_text, split_files

pytestmark = pytest.mark.gpu

PAIRS = {"rawA": R.synth_set(71, 2500, 0), "rawB": R.synth_set(72, 2000, 500)}


def texts_of(files):
    return {f.name: gzip.decompress(f.read_bytes()) for f in files}


def is_bgzf(data):
    from varkoder_amd import engine
    return engine.bgzf_members(data) is not None


def stats_without_times(path):
    import pandas as pd
    df = pd.read_csv(path)
    return df[[c for c in df.columns if not c.endswith("_time")]].sort_values("sample").reset_index(drop=True)


def test_from_clean_splits_with_and_without_the_flag(tmp_path):
    names = ["sampA", "sampB", "sampC"]
    for d in ("host", "gpu"):
        (tmp_path / d / "int" / "clean_reads").mkdir(parents=True)
        for i, s in enumerate(names):
            (tmp_path / d / "int" / "clean_reads" / f"{s}.fq.gz").write_bytes(gzip.compress(sample_text(100 + i), compresslevel=1))
    argv = ["--from-clean", "int", "-i", "int", "--write-splits", "-o", "A", "-f", "A.csv"] + COMMON
    run(argv, tmp_path / "host")
    run(argv + ["--gpu-gzip"], tmp_path / "gpu")
    host, gpu = split_files(tmp_path / "host" / "int"), split_files(tmp_path / "gpu" / "int")
    assert [f.name for f in host] == [f.name for f in gpu] and len(gpu) == 12
    assert texts_of(host) == texts_of(gpu)
    assert all(is_bgzf(f.read_bytes()) for f in gpu) and not any(is_bgzf(f.read_bytes()) for f in host)
    assert stats_without_times(tmp_path / "host" / "A.csv").equals(stats_without_times(tmp_path / "gpu" / "A.csv"))
    same_images(tmp_path / "host" / "A", tmp_path / "gpu" / "A")
    # the default entry on the flag's files: the direct run's images
    run(["int", "-o", "B", "-f", "B.csv"] + COMMON, tmp_path / "gpu")
    assert len(same_images(tmp_path / "gpu" / "A", tmp_path / "gpu" / "B")) == 12


def write_pairs(root, nested):
    for s, (r1, r2, se) in PAIRS.items():
        d = root / "tax" / s if nested else root / s
        d.mkdir(parents=True)
        (d / "lib_1.fq.gz").write_bytes(gzip.compress(R.fq(r1)))
        (d / "lib_2.fq.gz").write_bytes(gzip.compress(R.fq(r2)))
        if se:
            (d / "single.fastq").write_bytes(R.fq(se))


def test_from_raw_clean_reads_with_and_without_the_flag(tmp_path):
    for d in ("host", "gpu"):
        write_pairs(tmp_path / d / "raw", nested=True)
    argv = ["--from-raw", "raw", "-i", "int", "-o", "A", "-f", "A.csv"] + COMMON
    run(argv, tmp_path / "host")
    run(argv + ["--gpu-gzip"], tmp_path / "gpu")
    host = sorted((tmp_path / "host" / "int" / "clean_reads").glob("*.fq.gz"))
    gpu = sorted((tmp_path / "gpu" / "int" / "clean_reads").glob("*.fq.gz"))
    assert [f.name for f in host] == [f.name for f in gpu] == ["rawA.fq.gz", "rawB.fq.gz"]
    assert texts_of(host) == texts_of(gpu) and all(len(t) > 10000 for t in texts_of(gpu).values())
    assert all(is_bgzf(f.read_bytes()) for f in gpu)
    assert stats_without_times(tmp_path / "host" / "A.csv").equals(stats_without_times(tmp_path / "gpu" / "A.csv"))
    same_images(tmp_path / "host" / "A", tmp_path / "gpu" / "A")
    # a second run without -x takes the files as they are
    before = {f: f.stat().st_mtime_ns for f in gpu}
    run(["--from-raw", "raw", "-i", "int", "-o", "A2", "-f", "A2.csv", "--gpu-gzip"] + COMMON, tmp_path / "gpu")
    assert {f: f.stat().st_mtime_ns for f in gpu} == before
    same_images(tmp_path / "gpu" / "A", tmp_path / "gpu" / "A2")


def test_query_from_raw_with_and_without_the_flag(tmp_path):
    model_files(tmp_path)
    write_pairs(tmp_path / "raw", nested=False)
    common = ["-R", "5", "-M", "200M", "-b", "2", "-P"]
    query(tmp_path, tmp_path / "raw", tmp_path / "out_host", "--from-raw", "-i", tmp_path / "int_host", *common)
    query(tmp_path, tmp_path / "raw", tmp_path / "out_gpu", "--from-raw", "-i", tmp_path / "int_gpu", "--gpu-gzip", *common)
    a, b = ((tmp_path / d / "predictions.csv").read_text().replace(str(tmp_path / d), "") for d in ("out_host", "out_gpu"))
    assert a == b and a.count("\n") == 3
    host = texts_of(sorted((tmp_path / "int_host" / "clean_reads").glob("*.fq.gz")))
    assert host == texts_of(sorted((tmp_path / "int_gpu" / "clean_reads").glob("*.fq.gz"))) and len(host) == 2
