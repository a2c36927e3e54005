"""`--qc-report` end to end, on a folder of two tiny samples, one of them paired with single reads beside.  `image
--from-raw --qc-report DIR`: every `DIR/<sample>.qc.json` equals qc.report of tests/qc_ref.py's rows over the raw files
under the run's read budget and over tests/clean_ref.py's output, and the new stats.csv columns equal qc.columns of the
same; the same run without the flag writes the same pixels, cleaned reads, `_fastp_gpu.json` and old columns, and no
`.qc.json`; with --exclude-fasta the `after` part describes the kept reads; --from-clean, `query` (default entry and
--from-raw) and --from-bam write their reports.  Every refusal exits with 2 (no GPU needed for those)."""
import gzip
import json
from pathlib import Path

import numpy as np
import pytest

import bam_cases as BC
import bam_ref
import clean_ref as C
import qc_ref as R
import screen_ref
from test_gpu_query_raw import model_files, query
from test_gpu_write_splits import pngs, run
from varkoder_amd import qc, rawinput

gpu = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "5K", "-M", "20K", "-k", "7"]   # (-M: a budget of 100,000 bases, less than either sample holds)
MAX_BP = 20000
SETS = {"qcA": C.synth_set(85, 600, 400), "qcB": C.synth_set(86, 0, 1800)}
K = 25


def write_raw(root, nested):
    for s, (r1, r2, se) in SETS.items():
        d = root / "tax" / s if nested else root / s
        d.mkdir(parents=True)
        if r1:
            (d / "lib_1.fq.gz").write_bytes(gzip.compress(C.fq(r1)))
            (d / "lib_2.fq.gz").write_bytes(gzip.compress(C.fq(r2)))
        if se:
            (d / "single.fastq").write_bytes(C.fq(se))


def expected(sample, max_bp=MAX_BP, screen=None):
    """(before rows by role, after row, cleaned text) of a sample: the raw files under reads_needed's budget by the rule,
    the cleaned text clean_ref's (screen: a function of the text applied to it)."""
    r1, r2, se = SETS[sample]
    files = {"read1": ("R1", r1), "read2": ("R2", r2), "single": ("unpaired", se)}
    info = {"unpaired": [], "R1": [], "R2": []}
    for role, (key, recs) in files.items():
        if recs:
            info[key].append({"file": role, "avg_length": round(rawinput.avg_read_length(C.fq(recs))), "total_reads": len(recs)})
    take = rawinput.reads_needed(info, max_bp)
    before = {role: R.row(C.fq(recs), take.get(role, 0))[0] for role, (_, recs) in files.items() if recs}
    text = C.clean_sample(r1[:take.get("read1", 0)], r2[:take.get("read2", 0)], se[:take.get("single", 0)])[0]
    if screen is not None:
        text = screen(text)
    after, status = R.row(text, R.record_count(text))
    assert status == 0 and int(after[R.RECORDS]) > 100
    return before, after, text


def plain(obj):
    return json.loads(json.dumps(obj))


def read_stats(path):
    import pandas as pd
    return pd.read_csv(path, float_precision="round_trip").set_index("sample")


def check_columns(stats, sample, cols):
    for name, v in cols.items():
        assert float(stats.loc[sample, name]) == float(v), (sample, name)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """The raw folders and the run with the flag."""
    tmp = tmp_path_factory.mktemp("qc_cli")
    write_raw(tmp / "raw", nested=True)
    write_raw(tmp / "rawq", nested=False)
    run(["--from-raw", "raw", "-i", "int1", "-o", "img1", "-f", "s1.csv", "--qc-report", "qc1"] + COMMON, tmp)
    return tmp


@gpu
def test_image_from_raw_reports_equal_the_rule(base):
    tmp = base
    stats = read_stats(tmp / "s1.csv")
    assert sorted(p.name for p in (tmp / "qc1").iterdir()) == [f"{s}.qc.json" for s in sorted(SETS)]
    for s in SETS:
        before, after, text = expected(s)
        assert sum(int(r[R.RECORDS]) for r in before.values()) < sum(len(x) for x in SETS[s])   # (the budget bites)
        assert gzip.decompress((tmp / "int1" / "clean_reads" / f"{s}.fq.gz").read_bytes()) == text
        got = json.loads((tmp / "qc1" / f"{s}.qc.json").read_text())
        want = plain(qc.report(before, after))
        assert set(got) == set(want) == {"summary", "after_filtering"} | {f"{r}_before_filtering" for r in before}
        for key in want:
            assert got[key] == want[key], (s, key)
        check_columns(stats, s, qc.columns(qc.add_rows(before.values()), after))
    assert set(expected("qcA")[0]) == {"read1", "read2", "single"} and set(expected("qcB")[0]) == {"single"}


@gpu
def test_without_the_flag_nothing_differs(base):
    from PIL import Image
    tmp = base
    run(["--from-raw", "raw", "-i", "int0", "-o", "img0", "-f", "s0.csv"] + COMMON, tmp)
    a, b = pngs(tmp / "img0"), pngs(tmp / "img1")
    assert a and sorted(a) == sorted(b)
    for name in a:
        x, y = Image.open(a[name]), Image.open(b[name])
        assert np.array_equal(np.array(x), np.array(y)) and x.info == y.info, name
    for s in SETS:
        for name in (f"{s}.fq.gz", f"{s}_fastp_gpu.json"):
            x, y = ((tmp / d / "clean_reads" / name).read_bytes() for d in ("int0", "int1"))
            assert (gzip.decompress(x) == gzip.decompress(y)) if name.endswith(".gz") else x == y, name
    s0, s1 = read_stats(tmp / "s0.csv"), read_stats(tmp / "s1.csv")
    new = ["raw_reads", "raw_basepairs", "raw_q30_rate", "clean_reads", "clean_q30_rate", "clean_gc_content", "clean_mean_length"]
    assert [c for c in s1.columns if c not in new] == list(s0.columns) and [c for c in s1.columns if c in new] == new
    keep = [c for c in s0.columns if not c.endswith("_time")]
    import pandas as pd
    pd.testing.assert_frame_equal(s0[keep], s1[keep], check_exact=True)
    assert not [p for d in ("int0", "img0") for p in (tmp / d).rglob("*.qc.json")] and not list(tmp.glob("*.qc.json"))


def reference():
    """A FASTA of every tenth read of both samples (R1's and the single reads' sequences as they are)."""
    out = bytearray()
    for s, (r1, _, se) in SETS.items():
        for i, (_, seq, _) in enumerate((r1 or se)[::10]):
            out += b">%s_%d\n" % (s.encode(), i) + seq + b"\n"
    return bytes(out)


@gpu
def test_with_a_screen_the_after_part_describes_the_kept_reads(base):
    tmp = base
    fasta = reference()
    (tmp / "ref.fa").write_bytes(fasta)
    keys = screen_ref.set_ints(fasta, K)
    run(["--from-raw", "raw", "-o", "img2", "-f", "s2.csv", "--qc-report", "qc2", "--exclude-fasta", "ref.fa", "--screen-k", K] + COMMON,
        tmp)
    stats = read_stats(tmp / "s2.csv")
    for s in SETS:
        before, after, _ = expected(s, screen=lambda text: screen_ref.screen(text, keys, K, 1, False)[0])
        unscreened = expected(s)[1]
        assert 0 < int(after[R.RECORDS]) < int(unscreened[R.RECORDS])
        got = json.loads((tmp / "qc2" / f"{s}.qc.json").read_text())
        assert got == plain(qc.report(before, after)), s
        assert int(stats.loc[s, "clean_reads"]) == int(after[R.RECORDS]) == \
            int(stats.loc[s, "screen_reads_in"]) - int(stats.loc[s, "screen_reads_removed"])
        check_columns(stats, s, qc.columns(qc.add_rows(before.values()), after))


@gpu
def test_from_clean_and_query_write_their_reports(base):
    tmp = base
    # cleaned reads of the first run: the `after` sections only
    run(["--from-clean", "int1", "-o", "img3", "-f", "s3.csv", "--qc-report", "qc3"] + COMMON, tmp)
    stats = read_stats(tmp / "s3.csv")
    for s in SETS:
        _, after, _ = expected(s)
        got = json.loads((tmp / "qc3" / f"{s}.qc.json").read_text())
        assert got == plain(qc.report(None, after)) and set(got) == {"summary", "after_filtering"}, s
        check_columns(stats, s, qc.columns(None, after))
        assert "raw_reads" not in stats.columns
    model_files(tmp)
    common = ["-R", "5", "-M", "20K", "-b", "2", "-P"]
    query(tmp, tmp / "int1" / "clean_reads", tmp / "out4", "--qc-report", tmp / "qc4", *common)
    query(tmp, tmp / "rawq", tmp / "out5", "--from-raw", "--qc-report", tmp / "qc5", *common)
    for s in SETS:
        before, after, _ = expected(s)
        assert json.loads((tmp / "qc4" / f"{s}.qc.json").read_text()) == plain(qc.report(None, after)), s
        got = json.loads((tmp / "qc5" / f"{s}.qc.json").read_text())
        assert got == plain(qc.report(before, after)), s
        assert set(got) == {"summary", "after_filtering"} | {f"{r}_before_filtering" for r in before}
        assert set(got["summary"]) == {"before_filtering", "after_filtering"}


@gpu
def test_from_bam(tmp_path):
    """tests/bam_cases.py's bulk file: single reads, mates, reverse reads and excluded records mixed; every read a single read"""
    data = dict(BC.unit_cases())["bulk"]
    (tmp_path / "bam").mkdir()
    (tmp_path / "bam" / "bulk.bam").write_bytes(BC.bgzf(data))
    status, texts, _ = bam_ref.convert(data, bam_ref.header_end(data)[0])
    raw = texts[bam_ref.ALL]
    assert status == 0 and raw.count(b"\n") > 4000
    run(["--from-bam", "bam", "-o", "img", "-f", "s.csv", "--qc-report", "qc", "-R", "7", "-m", "5K", "-M", "0", "-k", "7"], tmp_path)
    before = {"single": R.row(raw, R.record_count(raw))[0]}
    text = C.clean_sample([], [], C.parse_fastq(raw))[0]
    after = R.row(text, R.record_count(text))[0]
    got = json.loads((tmp_path / "qc" / "bulk.qc.json").read_text())
    assert got == plain(qc.report(before, after))
    check_columns(read_stats(tmp_path / "s.csv"), "bulk", qc.columns(before["single"], after))


def test_refusals(tmp_path):
    """exit 2, before anything runs, naming the flag"""
    from varkoder_amd import cli
    q = ["query", "-l", "m.pt", "--vocab", "v.txt", "in", "out"]
    bad = [
        ["image", "in", "--qc-report", "qc"],                        # the default entry (step D)
        ["image", "in", "--from-fasta", "--qc-report", "qc"],
        ["image", "in", "--from-fasta", "--fragments", "--qc-report", "qc"],
        q + ["--from-fasta", "--qc-report", "qc"],
        q + ["--images", "--qc-report", "qc"],
        ["image", "in", "--from-raw", "--qc-report"],                # no folder
    ]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            cli.parse_args([str(a) for a in argv])
        assert e.value.code == 2, argv
    good = [
        ["image", "in", "--from-raw", "--qc-report", "qc"],
        ["image", "in", "--from-clean", "--qc-report", "qc"],
        ["image", "in", "--from-bam", "--bam-pairs", "--qc-report", "qc"],
        q + ["--qc-report", "qc"],
        q + ["--from-raw", "--qc-report", "qc"],
        q + ["--from-bam", "--qc-report", "qc"],
    ]
    for argv in good:
        assert cli.qc_options(cli.parse_args([str(a) for a in argv])) == Path("qc")
    args = cli.parse_args(["image", "in", "--from-raw"])
    assert cli.qc_options(args) is None and not hasattr(args, "qc_report")   # (opt-in: absent)


def test_a_refusal_names_the_flag(capsys):
    from varkoder_amd import cli
    with pytest.raises(SystemExit):
        cli.parse_args(["image", "in", "--qc-report", "qc"])
    assert "--qc-report" in capsys.readouterr().err
