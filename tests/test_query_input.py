"""`query --from-raw` off the GPU: the input table of a query against the reference's own process_input(is_query=True)
(tests/golden/query_input_cases.json, written by tools/gen_query_input_golden.py), the command line's new flags, and
the input errors that are raised before anything touches a device."""
import json
from pathlib import Path

import pytest

from varkoder_amd import cli, rawinput

GOLDEN = json.loads((Path(__file__).parent / "golden" / "query_input_cases.json").read_text())
RAW_GOLDEN = json.loads((Path(__file__).parent / "golden" / "raw_input_cases.json").read_text())
CASES = {c["name"]: c for c in GOLDEN["cases"]}


def make_tree(root, case):
    root.mkdir()
    for d in case.get("dirs", []):
        (root / d).mkdir(parents=True)
    for f in case["files"]:
        (root / f).parent.mkdir(parents=True, exist_ok=True)
        (root / f).write_bytes(b"")
    for link, target in case.get("links", {}).items():
        (root / link).symlink_to(root / target, target_is_directory=True)


def test_the_golden_file_holds_the_cases_the_feature_names():
    assert {"flat", "flat_pairs", "folders", "linked_folder", "mixed", "empty"} <= set(CASES)
    assert "exception" in CASES["empty"] and all("table" in CASES[n] for n in ("flat", "flat_pairs", "folders",
                                                                              "linked_folder", "mixed"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_query_input_matches_reference(tmp_path, name):
    case = CASES[name]
    root = tmp_path / "input"
    make_tree(root, case)
    if "exception" in case:
        # (the reference's own "no records read" check is never reached: pandas raises a KeyError on the empty table
        # first, which its caller turns into an input format error.  Here: the message of the check it meant.)
        with pytest.raises(Exception, match="no records read"):
            rawinput.process_input(root, is_query=True)
        return
    got = [[s, lab, [str(Path(f).relative_to(root)) for f in files]]
           for s, lab, files in rawinput.process_input(root, is_query=True)]
    assert got == case["table"]


def test_flat_folder_names_samples_up_to_the_first_dot(tmp_path):
    make_tree(tmp_path / "in", {"files": ["s_1.fq", "s_2.fq", "t.a.fq", "t.b.fq"]})
    got = rawinput.process_input(tmp_path / "in", is_query=True)
    assert [(s, lab, [Path(f).name for f in files]) for s, lab, files in got] == \
        [("s_1", ["query"], ["s_1.fq"]), ("s_2", ["query"], ["s_2.fq"]), ("t", ["query"], ["t.a.fq", "t.b.fq"])]


def test_non_query_input_is_unchanged_by_the_new_argument(tmp_path):
    root = tmp_path / "input"
    for d, files in RAW_GOLDEN["tree"].items():
        (root / d).mkdir(parents=True)
        for f in files:
            (root / d / f).write_bytes(b"")
    for f in RAW_GOLDEN["loose"]:
        (root / f).write_bytes(b"")
    for kw in ({}, {"is_query": False}):
        got = [[s, lab, [str(Path(f).relative_to(root)) for f in files]] for s, lab, files in rawinput.process_input(root, **kw)]
        assert got == RAW_GOLDEN["folder"]
    csv = tmp_path / "table" / "samples.csv"
    csv.parent.mkdir()
    csv.write_text(RAW_GOLDEN["csv_text"])
    got = [[s, lab, [str(Path(f).relative_to(csv.parent)) for f in files]]
           for s, lab, files in rawinput.process_input(csv, is_query=False)]
    assert got == RAW_GOLDEN["csv"]


BASE = ["query", "IN", "OUT", "-l", "m.pt", "--vocab", "v.txt"]


def test_query_from_raw_parses():
    args = cli.parse_args(BASE + ["--from-raw"])
    assert args.from_raw and not hasattr(args, "detect_adapters") and args.trim_bp == "10,10"
    args = cli.parse_args(BASE + ["--from-raw", "--detect-adapters", "--adapter-sequence", "AGATCGGAAGAGC"])
    assert args.detect_adapters and args.adapter_sequence == b"AGATCGGAAGAGC"
    assert not cli.parse_args(BASE).from_raw


@pytest.mark.parametrize("extra", (["--detect-adapters"], ["--adapter-sequence", "ACGTACGT"],
                                   ["--from-raw", "--detect-adapters", "-a"], ["--from-raw", "--adapter-sequence-r2", "ACGTACGT", "-a"],
                                   ["--from-raw", "--adapter-sequence", "ACG"], ["--from-raw", "--images"]))
def test_query_adapter_flags_are_refused_where_image_refuses_them(extra, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(BASE + extra)
    assert e.value.code == 2


def test_no_pairs_is_accepted_and_says_it_is_inert(capsys):
    assert cli.parse_args(BASE + ["--from-raw", "-1"]).no_pairs
    with pytest.raises(SystemExit):
        cli.parse_args(["query", "-h"])
    assert "inert" in capsys.readouterr().out


def test_from_raw_on_a_folder_of_images_asks_for_the_images_flag(tmp_path, monkeypatch):
    """Raised while the input is listed: no model is loaded and no engine made (either would fail here: the model
    file does not exist, and ImageEngine is replaced by something that raises)."""
    from varkoder_amd import engine
    monkeypatch.setattr(engine, "ImageEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU use")))
    src = tmp_path / "in"
    src.mkdir()
    (src / "s1.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    (src / "s1@00000001K+cgr+k7.png").write_bytes(b"")
    with pytest.raises(Exception, match="Use --images flag"):
        cli.main(["query", str(src), str(tmp_path / "out"), "-l", str(tmp_path / "none.pt"), "--vocab",
                  str(tmp_path / "none.txt"), "--from-raw"])
    assert not (tmp_path / "out").exists()


def test_from_raw_on_an_empty_folder_fails_before_any_gpu_use(tmp_path, monkeypatch):
    from varkoder_amd import engine
    monkeypatch.setattr(engine, "ImageEngine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU use")))
    (tmp_path / "in").mkdir()
    with pytest.raises(Exception, match="no records read"):
        cli.main(["query", str(tmp_path / "in"), str(tmp_path / "out"), "-l", "none.pt", "--vocab", "none.txt", "--from-raw"])


def test_seeds_follow_the_table_order(tmp_path):
    """str(row index) + str(rng draw), one draw per sample in table order (image.py:1017)."""
    import numpy as np
    make_tree(tmp_path / "in", {"files": ["b.fq", "a.fq", "c.fq.gz"]})
    ns = cli.parse_args(["query", str(tmp_path / "in"), "OUT", "-l", "m", "--vocab", "v", "--from-raw", "-R", "11"])
    plan = cli.RawPlan(ns, is_query=True)
    rng = np.random.default_rng(11)
    want = {s: int(str(i) + str(rng.integers(low=0, high=2 ** 32))) % (1 << 63) for i, s in enumerate(["a", "b", "c"])}
    assert plan.samples == ["a", "b", "c"] and plan.seeds == want and len(plan) == 3
    assert plan.raw == [(s, [str(tmp_path / "in" / f)]) for s, f in (("a", "a.fq"), ("b", "b.fq"), ("c", "c.fq.gz"))]
