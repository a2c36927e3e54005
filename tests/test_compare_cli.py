"""The `compare` command.  Without a GPU: the parser's refusals, the two CSV writers on hand-made (idx, d2), the
groups derived from file names.  With one: a folder of a dozen 32 x 32 PNG files compared with itself, with
--same-sample, --against and --matrix; every file written equals what tests/dist_ref.py and the writers give."""
import math
import os

import numpy as np
import pandas as pd
import pytest

import dist_ref
from varkoder_amd import cli, compare

NO_IDX, NO_D2 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


# ---- without a GPU --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv", [["compare", "in", "out", "-N", "0"], ["compare", "in", "out", "-N", "65"],
                                  ["compare", "in", "out", "--same-sample", "--against", "ref"], ["compare", "in"],
                                  ["compare", "in", "out", "--neighbours", "x"]])
def test_the_parser_refuses(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


def test_the_parser_defaults():
    a = cli.parse_args(["compare", "in", "out"])
    assert (a.command, a.input, a.outdir, a.neighbours, a.against, a.same_sample, a.matrix, a.overwrite) == \
        ("compare", "in", "out", 10, None, False, False, False)
    assert not hasattr(a, "gpu_png_read")
    a = cli.parse_args(["compare", "in", "out", "--against", "ref", "-N", "64", "--matrix", "-x", "--gpu-png-read", "-t", "l.csv"])
    assert (a.against, a.neighbours, a.matrix, a.overwrite, a.gpu_png_read, a.label_table) == ("ref", 64, True, True, True, "l.csv")


def test_an_existing_output_folder_is_refused_without_x(tmp_path, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    (tmp_path / "in").mkdir()
    (tmp_path / "out").mkdir()
    with pytest.raises(Exception, match="Output directory exists"):
        cli.main(["compare", str(tmp_path / "in"), str(tmp_path / "out")])


def test_a_world_above_one_is_refused(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    (tmp_path / "in").mkdir()
    with pytest.raises(Exception, match="one GPU"):
        cli.main(["compare", str(tmp_path / "in"), str(tmp_path / "out")])


def frame(rows):
    return pd.DataFrame([{"sample": s, "bp": bp, "img_kmer_mapping": "cgr", "img_kmer_size": 5,
                          "path": "dir/%s@%08dK+cgr+k5.png" % (s, bp // 1000), "labels": labels} for s, bp, labels in rows])


QDF = frame([("a", 1000, "genus:X;family:F"), ("a", 2000, "genus:X;family:F"), ("b", 1000, "genus:Y;family:F"), ("c", 1000, "")])
IDX = np.array([[2, 3, 1], [2, NO_IDX, NO_IDX], [0, 1, 3], [NO_IDX] * 3], dtype=np.uint32)
D2 = np.array([[0, 4 * 65025, 7], [1024, NO_D2, NO_D2], [0, 1024, 5000], [NO_D2] * 3], dtype=np.uint64)


def test_groups_come_from_the_file_names():
    from varkoder_amd.convert import get_metadata_from_img_filename
    names = ["s1@00000500K+cgr+k5.png", "s1@00001000K+cgr+k5.png", "s2@00000500K+cgr+k5.png", "s1@00002000K+cgr+k5.png",
             "s3@00000500K+cgr+k5.png"]
    df = pd.DataFrame([get_metadata_from_img_filename("x/" + n) for n in names])
    assert compare.groups_of(df).tolist() == [0, 0, 1, 0, 2] and compare.groups_of(df).dtype == np.uint32
    assert compare.groups_of(df, same_sample=True).tolist() == [0, 1, 2, 3, 4]


def test_the_neighbour_table():
    t = compare.neighbour_table(QDF, QDF, IDX, D2, 4)
    assert list(t.columns) == ["sample", "bp", "img_kmer_mapping", "img_kmer_size", "path", "labels", "rank", "neighbour_sample",
                               "neighbour_bp", "neighbour_path", "neighbour_labels", "sq_distance", "distance", "shared_labels"]
    assert len(t) == 3 + 1 + 3 + 0   # (fill slots produce no row)
    assert t["rank"].tolist() == [1, 2, 3, 1, 1, 2, 3]
    assert t["sample"].tolist() == ["a", "a", "a", "a", "b", "b", "b"] and t["bp"].tolist() == [1000, 1000, 1000, 2000, 1000, 1000, 1000]
    assert t["neighbour_sample"].tolist() == ["b", "c", "a", "b", "a", "a", "c"]
    assert t["neighbour_bp"].tolist() == [1000, 1000, 2000, 1000, 1000, 2000, 1000]
    assert t["neighbour_path"][0] == "dir/b@00000001K+cgr+k5.png" and t["path"][0] == "dir/a@00000001K+cgr+k5.png"
    assert t["sq_distance"].tolist() == [0, 260100, 7, 1024, 0, 1024, 5000]
    # distance = sqrt(sq / P) / 255: every pixel a full range apart is 1
    assert t["distance"][0] == 0.0 and t["distance"][1] == 1.0
    assert t["distance"][2] == math.sqrt(7 / 4) / 255 and t["distance"][3] == math.sqrt(1024 / 4) / 255
    assert t["shared_labels"].tolist() == ["family:F", "", "family:F;genus:X", "family:F", "family:F", "family:F", ""]


def test_the_sample_table():
    t = compare.sample_table(QDF, QDF, IDX, D2, 4)
    assert list(t.columns) == ["sample", "bp", "path", "labels", "nearest_distance", "majority_labels", "own_labels_in_majority"]
    assert len(t) == 4
    # a@1000: neighbours b, c, a@2000: family:F on 2 of 3 (more than half), genus:X and genus:Y on 1 each
    assert t["majority_labels"].tolist() == ["family:F", "family:F;genus:Y", "family:F;genus:X", ""]
    assert t["own_labels_in_majority"].tolist() == [0.5, 0.5, 0.5, ""]
    assert t["nearest_distance"].tolist() == [0.0, math.sqrt(1024 / 4) / 255, 0.0, ""]
    # exactly half is no majority
    half = compare.sample_table(QDF[:1], QDF, np.array([[0, 2]], dtype=np.uint32), np.array([[1, 2]], dtype=np.uint64), 4)
    assert half["majority_labels"].tolist() == ["family:F"] and half["own_labels_in_majority"].tolist() == [0.5]


# ---- with a GPU -----------------------------------------------------------------------------------------------------

SPEC = [("s1", 500, "genus:A;family:F"), ("s1", 1000, "genus:A;family:F"), ("s2", 500, "genus:A;family:F"),
        ("s2", 1000, "genus:A;family:F"), ("s3", 500, "genus:B;family:G"), ("s3", 1000, "genus:B;family:G"),
        ("dup1", 500, "genus:C"), ("dup2", 500, "species:D"), ("s4", 500, "genus:B;family:G"), ("s5", 500, "genus:A"),
        ("s6", 500, ""), ("s7", 500, "genus:B;family:F")]


def write_folder(d, spec, seed):
    from varkoder_amd.image import write_png
    g = np.random.default_rng(seed)
    base = {}
    os.makedirs(d, exist_ok=True)
    for s, bp, labels in spec:
        if s.startswith("dup"):
            arr = base.setdefault("dup", g.integers(0, 256, (32, 32), dtype=np.uint8))   # exact duplicates
        else:
            b = base.setdefault(s, g.integers(0, 256, (32, 32), dtype=np.int64))
            arr = np.clip(b + g.integers(-20, 21, (32, 32)), 0, 255).astype(np.uint8)     # a sample's steps resemble each other
        write_png(arr, os.path.join(d, "%s@%08dK+cgr+k5.png" % (s, bp)), [x for x in labels.split(";") if x], 0.01, 0.1, "cgr")


def expected_tables(qdir, rdir, n, groups):
    """(neighbours, samples, matrix, qdf, rdf) by train's collection, PIL, tests/dist_ref.py and the writers."""
    from PIL import Image
    from varkoder_amd.train import collect_images
    qdf = collect_images(qdir).reset_index(drop=True)
    rdf = collect_images(rdir).reset_index(drop=True) if rdir else qdf
    px = lambda df: np.stack([np.array(Image.open(p)) for p in df["path"]]).reshape(len(df), -1)   # noqa: E731
    m = dist_ref.matrix(px(qdf), px(rdf))
    g = None if groups is None else compare.groups_of(qdf, groups == "image")
    idx, d2 = dist_ref.neighbours(m, n, g, g)
    return compare.neighbour_table(qdf, rdf, idx, d2, 1024), compare.sample_table(qdf, rdf, idx, d2, 1024), m, qdf, rdf


def same_csv(path, table):
    with open(path) as f:
        return f.read() == table.to_csv(index=False)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    d = tmp_path_factory.mktemp("compare")
    write_folder(str(d / "images"), SPEC, 5)
    write_folder(str(d / "refs"), SPEC[2:9], 6)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("flags, groups", [([], "sample"), (["--same-sample"], "image"), (["--gpu-png-read", "-N", "3"], "sample")])
def test_compare_a_folder_with_itself(folders, flags, groups):
    out = folders / ("self_" + "_".join(f.strip("-") for f in flags))
    cli.main(["compare", str(folders / "images"), str(out)] + flags)
    n = 3 if "-N" in flags else 10
    neighbours, samples, _, qdf, _ = expected_tables(str(folders / "images"), None, n, groups)
    assert len(qdf) == 12
    assert same_csv(out / "neighbours.csv", neighbours) and same_csv(out / "samples.csv", samples)
    assert not (out / "distances.npy").exists()
    got = pd.read_csv(out / "neighbours.csv", keep_default_na=False)
    # the duplicates are each other's rank 1 at distance 0, and share no label
    for a, b in (("dup1", "dup2"), ("dup2", "dup1")):
        row = got[(got["sample"] == a) & (got["rank"] == 1)].iloc[0]
        assert (row["neighbour_sample"], row["sq_distance"], row["distance"], row["shared_labels"]) == (b, 0, 0.0, "")
    # an image's own sample is among its neighbours only with --same-sample, the image itself never
    own = got[got["sample"] == got["neighbour_sample"]]
    assert (len(own) > 0) == (groups == "image") and not (got["path"] == got["neighbour_path"]).any()
    if groups == "image":
        assert got[(got["sample"] == "s1") & (got["bp"] == 500000) & (got["rank"] == 1)].iloc[0]["neighbour_bp"] == 1000000
    assert len(got) == 12 * n   # (every image has at least ten others to choose from)


@pytest.mark.gpu
def test_compare_against_references_with_the_matrix(folders):
    out = folders / "against"
    cli.main(["compare", str(folders / "images"), str(out), "--against", str(folders / "refs"), "--matrix", "-N", "4"])
    neighbours, samples, m, qdf, rdf = expected_tables(str(folders / "images"), str(folders / "refs"), 4, None)
    assert same_csv(out / "neighbours.csv", neighbours) and same_csv(out / "samples.csv", samples)
    assert len(neighbours) == 12 * 4   # (no exclusions)
    got = np.load(out / "distances.npy")
    assert got.dtype == np.uint64 and got.shape == (12, 7) and np.array_equal(got, m)
    assert (out / "distances_rows.txt").read_text().split("\n")[:-1] == [str(p) for p in qdf["path"]]
    assert (out / "distances_cols.txt").read_text().split("\n")[:-1] == [str(p) for p in rdf["path"]]
    # again into the same folder: refused without -x, done with it
    with pytest.raises(Exception, match="Output directory exists"):
        cli.main(["compare", str(folders / "images"), str(out)])
    cli.main(["compare", str(folders / "images"), str(out), "-x", "--matrix"])
    assert np.array_equal(np.load(out / "distances.npy"), expected_tables(str(folders / "images"), None, 10, "sample")[2])


@pytest.mark.gpu
def test_sizes_that_differ_between_the_folders_are_refused(folders, tmp_path):
    from varkoder_amd.image import write_png
    os.makedirs(tmp_path / "big")
    write_png(np.zeros((64, 64), dtype=np.uint8), str(tmp_path / "big" / "z@00000500K+cgr+k6.png"), ["genus:Z"], 0.01, 0.1, "cgr")
    with pytest.raises(Exception, match="Images of different sizes"):
        cli.main(["compare", str(folders / "images"), str(tmp_path / "out"), "--against", str(tmp_path / "big")])
