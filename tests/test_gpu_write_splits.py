"""`image --write-splits`: the subsample ladder's reads go to <int>/split_fastqs/, and the default entry on those
files gives the images of the direct run."""
import gzip
import os
import random
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "5K", "-M", "50K", "-k", "7"]


def run(argv, cwd):
    """`python -m varkoder_amd image ...` in this process (a run is one engine; no second interpreter to start)."""
    from varkoder_amd import cli
    old = os.getcwd()
    os.chdir(cwd)
    try:
        cli.main(["image"] + [str(a) for a in argv])
    finally:
        os.chdir(old)


def sample_text(seed, bases=60000):
    rng = random.Random(seed)
    parts, total, i = [], 0, 0
    while total < bases:
        n = rng.choice((150, 150, 150, 150, 120, 640, 1230))
        seq = "".join(rng.choice("ACGT") for _ in range(n))
        parts.append(f"@s{seed}.{i} extra\n{seq}\n+\n{'G' * n}\n")
        total += n
        i += 1
    return "".join(parts).encode()


def pngs(folder):
    return {p.name: p for p in Path(folder).rglob("*.png")}


def same_images(a, b):
    from PIL import Image
    fa, fb = pngs(a), pngs(b)
    assert fa and sorted(fa) == sorted(fb)
    for name in fa:
        ia, ib = Image.open(fa[name]), Image.open(fb[name])
        assert np.array_equal(np.array(ia), np.array(ib)), name
        assert ia.info == ib.info, name
    return sorted(fa)


def split_files(int_dir):
    d = Path(int_dir) / "split_fastqs"
    return sorted(d.iterdir()) if d.is_dir() else []


def check_splits(int_dir, stats_csv, samples):
    """every file gunzips to FASTQ; the names carry the sizes stats.csv lists for the sample"""
    import pandas as pd
    stats = pd.read_csv(stats_csv).set_index("sample")
    files = split_files(int_dir)
    for s in samples:
        want = [str(int(int(bp) / 1000)).rjust(8, "0") for bp in str(stats.loc[s, "splitting_bp_per_file"]).split(",")]
        got = sorted((f.name.split("@")[1].removesuffix("K.fq.gz") for f in files if f.name.startswith(s + "@")), reverse=True)
        assert got == want and len(got) == 4, s
    for f in files:
        text = gzip.decompress(f.read_bytes())
        assert text.startswith(b"@") and text.count(b"\n") % 4 == 0, f.name
    return stats


@pytest.fixture(scope="module")
def clean_int(tmp_path_factory):
    """an intermediate folder with three cleaned samples, and the run that wrote their splits and images"""
    tmp = tmp_path_factory.mktemp("splits_clean")
    names = ["sampA", "sampB", "sampC"]
    (tmp / "int" / "clean_reads").mkdir(parents=True)
    for i, s in enumerate(names):
        (tmp / "int" / "clean_reads" / f"{s}.fq.gz").write_bytes(gzip.compress(sample_text(100 + i), compresslevel=1))
    run(["--from-clean", "int", "-i", "int", "--write-splits", "-o", "A", "-f", "A.csv"] + COMMON, tmp)
    return tmp, names


def test_from_clean_round_trip(clean_int):
    tmp, names = clean_int
    stats = check_splits(tmp / "int", tmp / "A.csv", names)
    run(["int", "-o", "B", "-f", "B.csv"] + COMMON, tmp)
    assert len(same_images(tmp / "A", tmp / "B")) == 12
    # the direct run without the flag: the same images and sizes, and no folder
    (tmp / "plain").mkdir()
    for f in (tmp / "int" / "clean_reads").iterdir():
        (tmp / "plain" / f.name).write_bytes(f.read_bytes())
    run(["--from-clean", "plain", "-i", "int2", "-o", "C", "-f", "C.csv"] + COMMON, tmp)
    same_images(tmp / "A", tmp / "C")
    import pandas as pd
    plain = pd.read_csv(tmp / "C.csv").set_index("sample")
    assert plain["splitting_bp_per_file"].to_dict() == stats["splitting_bp_per_file"].to_dict()
    assert not split_files(tmp / "int2")


def test_a_second_run_keeps_the_files(clean_int):
    tmp, names = clean_int
    before = {f: f.stat().st_mtime_ns for f in split_files(tmp / "int")}
    assert len(before) == 12
    run(["--from-clean", "int", "-i", "int", "--write-splits", "-o", "A2", "-f", "A2.csv"] + COMMON, tmp)
    assert {f: f.stat().st_mtime_ns for f in split_files(tmp / "int")} == before
    same_images(tmp / "A", tmp / "A2")
    # -x writes them again, with the same bytes inside
    texts = {f: gzip.decompress(f.read_bytes()) for f in before}
    run(["--from-clean", "int", "-i", "int", "--write-splits", "-x", "-o", "A2", "-f", "A2.csv"] + COMMON, tmp)
    after = split_files(tmp / "int")
    assert sorted(after) == sorted(before) and any(f.stat().st_mtime_ns != before[f] for f in after)
    assert {f: gzip.decompress(f.read_bytes()) for f in after} == texts


def test_no_image_writes_the_intermediates_only(clean_int, tmp_path):
    src, names = clean_int
    (tmp_path / "int" / "clean_reads").mkdir(parents=True)
    for f in (src / "int" / "clean_reads").iterdir():
        (tmp_path / "int" / "clean_reads" / f.name).write_bytes(f.read_bytes())
    run(["--from-clean", "int", "-i", "int", "--write-splits", "-X", "-o", "X", "-f", "X.csv"] + COMMON, tmp_path)
    stats = check_splits(tmp_path / "int", tmp_path / "X.csv", names)
    assert not pngs(tmp_path / "X")
    assert "7mer_counting_time" not in stats.columns and (stats["splitting_time"] > 0).all()
    got = {f.name: gzip.decompress(f.read_bytes()) for f in split_files(tmp_path / "int")}
    assert got == {f.name: gzip.decompress(f.read_bytes()) for f in split_files(src / "int")}


def test_from_raw_round_trip(tmp_path):
    import pandas as pd
    plan = [("taxA", "rawA"), ("taxB", "rawB"), ("taxB", "rawC")]
    for i, (taxon, s) in enumerate(plan):
        d = tmp_path / "raw" / taxon / s
        d.mkdir(parents=True)
        (d / f"{s}.fq").write_bytes(sample_text(200 + i, bases=80000))
    pd.DataFrame({"sample": [s for _, s in plan], "labels": [t for t, _ in plan]}).to_csv(tmp_path / "labels.csv", index=False)
    run(["--from-raw", "raw", "-i", "int", "--write-splits", "-o", "A", "-f", "A.csv"] + COMMON, tmp_path)
    check_splits(tmp_path / "int", tmp_path / "A.csv", [s for _, s in plan])
    run(["int", "-o", "B", "-f", "B.csv", "--labels-csv", "labels.csv"] + COMMON, tmp_path)
    assert len(same_images(tmp_path / "A", tmp_path / "B")) == 12


def test_the_flag_needs_its_entry_and_its_folder(tmp_path, capsys):
    """(the message tells the flag's own rule from argparse's unknown flag, which exits with 2 as well)"""
    (tmp_path / "in").mkdir()
    for argv, said in ((["in", "--write-splits", "-i", "int"], "only with --from-raw or --from-clean"),
                       (["--from-clean", "in", "--write-splits"], "needs -i"),
                       (["--from-raw", "in", "--write-splits"], "needs -i")):
        with pytest.raises(SystemExit) as err:
            run(argv + ["-o", "out"], tmp_path)
        assert err.value.code == 2
        assert "--write-splits: " + said in capsys.readouterr().err
    assert not (tmp_path / "out").exists() and not (tmp_path / "int").exists()
