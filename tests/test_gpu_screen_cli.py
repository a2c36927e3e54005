"""`--exclude-fasta` / `--keep-fasta` end to end, on a folder of two tiny samples, one of them paired.
Run A: `image --from-raw -i INT` without the screen, its clean_reads filtered on the host with tests/screen_ref.py, `image
--from-clean` on the filtered files.  Run B: one `image --from-raw --exclude-fasta REF.fa.gz` run.  The pixels of A and B are
equal, B's clean_reads are A's filtered files, and the new stats columns and the JSON object hold screen_ref's counts; the
same with --keep-fasta, and with `query --from-raw` on the rows of predictions.csv.  Every refusal exits with 2 (no GPU
needed for those)."""
import gzip
import json
import shutil
from pathlib import Path

import numpy as np
import pytest

import clean_ref as C
import screen_ref as R
from test_gpu_query_raw import model_files, query
from test_gpu_write_splits import COMMON, pngs, run

gpu = pytest.mark.gpu

K = 25
SETS = {"rawA": C.synth_set(81, 1500, 0), "rawB": C.synth_set(82, 0, 1800)}


def write_raw(root, nested):
    for s, (r1, r2, se) in SETS.items():
        d = root / "tax" / s if nested else root / s
        d.mkdir(parents=True)
        if r1:
            (d / "lib_1.fq.gz").write_bytes(gzip.compress(C.fq(r1)))
            (d / "lib_2.fq.gz").write_bytes(gzip.compress(C.fq(r2)))
        if se:
            (d / "single.fastq").write_bytes(C.fq(se))


def reference():
    """A FASTA of every tenth read of both samples (R1's and the single reads' sequences as they are: N's, adapters and
    poly-G included), wrapped at 70, two of the records joined by a run of N."""
    recs = []
    for s, (r1, _, se) in SETS.items():
        for i, (_, seq, _) in enumerate((r1 or se)[::10]):
            recs.append((b"%s_%d" % (s.encode(), i), seq))
    recs[0] = (b"joined", recs[0][1] + b"NNNN" + recs[1][1])
    out = bytearray()
    for name, seq in recs:
        out += b">" + name + b" a reference record\n"
        for i in range(0, len(seq), 70):
            out += seq[i:i + 70] + b"\n"
    return bytes(out)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """The raw folders, the reference, and run A's first half: the unscreened clean_reads."""
    tmp = tmp_path_factory.mktemp("screen_cli")
    write_raw(tmp / "raw", nested=True)
    write_raw(tmp / "rawq", nested=False)
    fasta = reference()
    (tmp / "ref.fa.gz").write_bytes(gzip.compress(fasta))
    (tmp / "ref.fa").write_bytes(fasta)
    run(["--from-raw", "raw", "-i", "int0", "-o", "img0", "-f", "s0.csv"] + COMMON, tmp)
    clean = {s: gzip.decompress((tmp / "int0" / "clean_reads" / f"{s}.fq.gz").read_bytes()) for s in SETS}
    assert all(len(t) > 20000 for t in clean.values())
    return tmp, fasta, clean, R.set_ints(fasta, K)


def filtered_folder(tmp, name, clean, keys, keep, source="int0"):
    """run A's second half: clean_reads filtered on the host (the reports beside them as they are); -> {sample: (text,
    stats)}"""
    d = tmp / name / "clean_reads"
    d.mkdir(parents=True)
    want = {}
    for s, text in clean.items():
        out, stats, status = R.screen(text, keys, K, 1, keep)
        assert status == 0 and 0 < stats[1] < stats[0]
        (d / f"{s}.fq.gz").write_bytes(gzip.compress(out, compresslevel=1))
        shutil.copy(tmp / source / "clean_reads" / f"{s}_fastp_gpu.json", d / f"{s}_fastp_gpu.json")
        want[s] = (out, stats)
    return want


def same_pixels(a, b):
    from PIL import Image
    fa, fb = pngs(a), pngs(b)
    assert fa and sorted(fa) == sorted(fb)
    for name in fa:
        assert np.array_equal(np.array(Image.open(fa[name])), np.array(Image.open(fb[name]))), name
    return sorted(fa)


@gpu
@pytest.mark.parametrize("keep", (False, True))
def test_image_from_raw_screened_equals_the_host_filter(base, keep):
    import pandas as pd
    tmp, fasta, clean, keys = base
    tag = "keep" if keep else "excl"
    want = filtered_folder(tmp, "filt_" + tag, clean, keys, keep)
    run(["--from-clean", "filt_" + tag, "-o", "A_" + tag, "-f", f"A_{tag}.csv"] + COMMON, tmp)
    flag = ["--keep-fasta", "ref.fa"] if keep else ["--exclude-fasta", "ref.fa.gz"]
    run(["--from-raw", "raw", "-i", "int_" + tag, "-o", "B_" + tag, "-f", f"B_{tag}.csv", "--screen-k", K] + flag + COMMON, tmp)
    names = same_pixels(tmp / ("A_" + tag), tmp / ("B_" + tag))
    assert {n.split("@")[0] for n in names} == set(SETS)
    stats = pd.read_csv(tmp / f"B_{tag}.csv").set_index("sample")
    plain = pd.read_csv(tmp / "s0.csv").set_index("sample")
    assert not [c for c in plain.columns if c.startswith("screen_")]   # (without the flags: no column)
    for s, (text, st) in want.items():
        assert gzip.decompress((tmp / ("int_" + tag) / "clean_reads" / f"{s}.fq.gz").read_bytes()) == text
        assert int(stats.loc[s, "screen_reads_in"]) == st[0]
        assert int(stats.loc[s, "screen_reads_removed"]) == st[0] - st[1]
        assert int(stats.loc[s, "screen_basepairs_removed"]) == st[2] - st[3]
        assert stats.loc[s, "clean_basepairs"] == plain.loc[s, "clean_basepairs"]   # (the cleaning's, before the screen)
        rep = json.loads((tmp / ("int_" + tag) / "clean_reads" / f"{s}_fastp_gpu.json").read_text())
        assert rep["screen"] == {"reference": "ref.fa" if keep else "ref.fa.gz", "k": K, "min_hits": 1,
                                 "mode": "keep" if keep else "exclude", "distinct_kmers": len(keys),
                                 "screen_reads_in": st[0], "screen_reads_removed": st[0] - st[1],
                                 "screen_basepairs_removed": st[2] - st[3]}
        base_rep = json.loads((tmp / "int0" / "clean_reads" / f"{s}_fastp_gpu.json").read_text())
        assert "screen" not in base_rep and rep["read1_after_filtering"] == base_rep["read1_after_filtering"]
    # a later --from-clean run on the screened folder reproduces the images
    run(["--from-clean", "int_" + tag, "-o", "C_" + tag, "-f", f"C_{tag}.csv"] + COMMON, tmp)
    same_pixels(tmp / ("B_" + tag), tmp / ("C_" + tag))
    # --from-clean with the flag on the UNSCREENED folder: the same again
    run(["--from-clean", "int0", "-o", "D_" + tag, "-f", f"D_{tag}.csv", "--screen-k", K] + flag + COMMON, tmp)
    same_pixels(tmp / ("B_" + tag), tmp / ("D_" + tag))
    d = pd.read_csv(tmp / f"D_{tag}.csv").set_index("sample")
    assert all(int(d.loc[s, "screen_reads_removed"]) == st[0] - st[1] for s, (_, st) in want.items())


@gpu
def test_query_from_raw_screened_equals_the_host_filter(base):
    tmp, fasta, _, keys = base
    model_files(tmp)
    common = ["-R", "5", "-M", "200M", "-b", "2", "-P"]
    # run A: the query's own cleaning (its read budget is -M's) without the screen, filtered on the host; the filtered
    # files are then taken as an earlier run's clean_reads
    query(tmp, tmp / "rawq", tmp / "out0", "--from-raw", "-i", tmp / "intq", *common)
    clean = {s: gzip.decompress((tmp / "intq" / "clean_reads" / f"{s}.fq.gz").read_bytes()) for s in SETS}
    filtered_folder(tmp, "filt_q", clean, keys, False, source="intq")
    query(tmp, tmp / "rawq", tmp / "outA", "--from-raw", "-i", tmp / "filt_q", *common)
    query(tmp, tmp / "rawq", tmp / "outB", "--from-raw", "--exclude-fasta", tmp / "ref.fa.gz", "--screen-k", K, *common)
    a, b = ((tmp / d / "predictions.csv").read_text().replace(str(tmp / d), "") for d in ("outA", "outB"))
    assert a == b and a.count("\n") == 3
    # the cleaned reads of an earlier run, screened as they are uploaded
    query(tmp, tmp / "intq" / "clean_reads", tmp / "outC", "--exclude-fasta", tmp / "ref.fa", "--screen-k", K, *common)
    query(tmp, tmp / "filt_q" / "clean_reads", tmp / "outD", *common)
    c, d = ((tmp / x / "predictions.csv").read_text().replace(str(tmp / x), "") for x in ("outC", "outD"))
    assert c == d and c.count("\n") == 3


def test_refusals(tmp_path):
    """exit 2, before anything runs"""
    from varkoder_amd import cli
    ref = tmp_path / "ref.fa"
    ref.write_bytes(b">r\nACGT\n")
    q = ["query", "-l", "m.pt", "--vocab", "v.txt", "in", "out"]
    bad = [
        ["image", "in", "--exclude-fasta", ref],                                       # the default entry (step D)
        ["image", "in", "--keep-fasta", ref],
        ["image", "in", "--from-fasta", "--exclude-fasta", ref],
        ["image", "in", "--from-fasta", "--keep-fasta", ref],
        q + ["--from-fasta", "--exclude-fasta", ref],
        q + ["--images", "--exclude-fasta", ref],
        q + ["--images", "--keep-fasta", ref],
        ["image", "in", "--from-raw", "--screen-k", "21"],                             # without one of the two flags
        ["image", "in", "--from-raw", "--screen-min-hits", "2"],
        q + ["--from-raw", "--screen-k", "21"],
        q + ["--screen-min-hits", "2"],
        ["image", "in", "--from-raw", "--exclude-fasta", ref, "--keep-fasta", ref],    # both
        q + ["--exclude-fasta", ref, "--keep-fasta", ref],
        ["image", "in", "--from-raw", "--exclude-fasta", ref, "--screen-k", "15"],
        ["image", "in", "--from-clean", "--keep-fasta", ref, "--screen-k", "32"],
        q + ["--exclude-fasta", ref, "--screen-k", "0"],
        ["image", "in", "--from-raw", "--exclude-fasta", ref, "--screen-min-hits", "0"],
        q + ["--from-raw", "--keep-fasta", ref, "--screen-min-hits", "-1"],
        ["image", "in", "--from-raw", "--exclude-fasta", tmp_path / "missing.fa"],     # a reference that does not exist
        ["image", "in", "--from-bam", "--keep-fasta", tmp_path / "missing.fa"],
        q + ["--exclude-fasta", tmp_path],                                             # (a folder is no file)
    ]
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            cli.parse_args([str(a) for a in argv])
        assert e.value.code == 2, argv
    good = [
        ["image", "in", "--from-raw", "--exclude-fasta", ref],
        ["image", "in", "--from-clean", "--keep-fasta", ref, "--screen-k", "16", "--screen-min-hits", "3"],
        ["image", "in", "--from-bam", "--bam-pairs", "--bam-read-groups", "--exclude-fasta", ref, "--screen-k", "31"],
        q + ["--exclude-fasta", ref],
        q + ["--from-raw", "--keep-fasta", ref],
        q + ["--from-bam", "--exclude-fasta", ref],
    ]
    for argv in good:
        args = cli.parse_args([str(a) for a in argv])
        s = cli.screen_options(args)
        assert s is not None and s.keep == ("--keep-fasta" in argv) and Path(s.fasta) == ref
    args = cli.parse_args(["image", "in", "--from-raw"])
    assert cli.screen_options(args) is None
    assert not [n for n in ("exclude_fasta", "keep_fasta", "screen_k", "screen_min_hits") if hasattr(args, n)]   # (opt-in: absent)
