"""`image --from-bam` and `query --from-bam` end to end on the GPU: BAM files written from synthetic reads (tests/bam_cases.py)
give what `--from-raw` gives for the same reads as FASTQ files -- PNG bytes, stats.csv rows (timing columns apart), the
reads of split_fastqs/, predictions.csv -- with reverse-flagged records restored, secondary copies dropped, mates split
into R1 and R2 by --bam-pairs; and a BAM whose last record is cut short fails its own sample only."""
import gzip
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_cases as BC  # noqa: E402
import clean_ref as R  # noqa: E402
from test_gpu_query_raw import VOCAB, model_files  # noqa: E402

pytestmark = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "50K", "-M", "200K", "-k", "7"]
CODES = {c: i for i, c in enumerate(BC.CODES)}


def run(command, argv, cwd):
    from varkoder_amd import cli
    old = os.getcwd()
    os.chdir(cwd)
    try:
        cli.main([command] + [str(a) for a in argv])
    finally:
        os.chdir(old)


def bare(records):
    """clean_ref records with names a BAM would hold (no comment behind a blank)."""
    return [(h.split(b" ")[0], s, q) for h, s, q in records]


def bam_record(rec, flag=4, reverse=False, **kw):
    """A clean_ref record (header line, sequence, quality text) as a BAM record; reverse: stored as an aligner stores a
    read of the reverse strand (reverse complement, qualities reversed, flag 0x10)."""
    h, s, q = rec
    seq, qual = s.decode(), [c - 33 for c in q]
    if reverse:
        seq, qual, flag = R.revcomp(s).decode(), qual[::-1], flag | 0x10
    return BC.record(h[1:], seq, qual, flag=flag, **kw)


# three samples of about 2,000 single reads: as they are; every third stored from the reverse strand; with secondary and
# supplementary copies in between
READS = {"s1": bare(R.synth_set(71, 0, 2000)[2]), "s2": bare(R.synth_set(72, 0, 2100)[2]), "s3": bare(R.synth_set(73, 0, 1900)[2])}
LABELS = {"s1": "taxA", "s2": "taxB", "s3": "taxB"}
HEAD = BC.header(BC.HD_UNSORTED, BC.REFS3)


def sample_bam(s):
    recs = []
    for i, rec in enumerate(READS[s]):
        if s == "s2" and i % 3 == 0:
            recs.append(bam_record(rec, flag=0, reverse=True, ref_id=1, pos=100 + i, cigar=(len(rec[1]) << 4,)))
        else:
            recs.append(bam_record(rec))
        if s == "s3" and i % 4 == 0:
            recs.append(bam_record(rec, flag=0x100 if i % 8 else 0x800, ref_id=0, pos=i, cigar=(len(rec[1]) << 4,)))
    return BC.bgzf(BC.inflated(recs, HEAD))


def write_inputs(tmp):
    import pandas as pd
    (tmp / "bam").mkdir()
    for s in READS:
        (tmp / "bam" / f"{s}.bam").write_bytes(sample_bam(s))
        d = tmp / "raw" / LABELS[s] / s
        d.mkdir(parents=True)
        (d / f"{s}.fq").write_bytes(R.fq(READS[s]))
    pd.DataFrame({"sample": list(READS), "labels": [LABELS[s] for s in READS]}).to_csv(tmp / "labels.csv", index=False)


def same_outputs(tmp, a, b):
    """Images byte for byte, stats rows but for the timing columns, the reads of every split file."""
    import pandas as pd
    pa = {p.name: p for p in (tmp / a).rglob("*.png")}
    pb = {p.name: p for p in (tmp / b).rglob("*.png")}
    assert pa and sorted(pa) == sorted(pb)
    for name in pa:
        assert pa[name].read_bytes() == pb[name].read_bytes(), name
    sa, sb = pd.read_csv(tmp / f"{a}.csv"), pd.read_csv(tmp / f"{b}.csv")
    keep = [c for c in sa.columns if not c.endswith("_time")]
    assert list(sa.columns) == list(sb.columns) and "clean_basepairs" in keep
    pd.testing.assert_frame_equal(sa[keep], sb[keep], check_exact=True)
    fa = sorted((tmp / f"int_{a}" / "split_fastqs").iterdir())
    fb = sorted((tmp / f"int_{b}" / "split_fastqs").iterdir())
    assert fa and [f.name for f in fa] == [f.name for f in fb]
    for x, y in zip(fa, fb):
        assert gzip.decompress(x.read_bytes()) == gzip.decompress(y.read_bytes()), x.name
    for s in sa["sample"]:
        x, y = (tmp / f"int_{n}" / "clean_reads" / f"{s}.fq.gz" for n in (a, b))
        assert gzip.decompress(x.read_bytes()) == gzip.decompress(y.read_bytes()), s
    return sorted(pa)


def test_image_from_bam_equals_from_raw(tmp_path):
    write_inputs(tmp_path)
    run("image", ["bam", "--from-bam", "--labels-csv", "labels.csv", "-i", "int_A", "--write-splits", "-o", "A", "-f", "A.csv"] + COMMON,
        tmp_path)
    run("image", ["raw", "--from-raw", "-i", "int_B", "--write-splits", "-o", "B", "-f", "B.csv"] + COMMON, tmp_path)
    names = same_outputs(tmp_path, "A", "B")
    assert {n.split("@")[0] for n in names} == set(READS)


def test_bam_pairs_equals_r1_r2_files(tmp_path):
    r1, r2, _ = R.synth_set(74, 1000, 0)
    r1, r2 = bare(r1), bare(r2)
    extra = bare(R.synth_set(75, 0, 300)[2])
    recs = []
    for i, (a, b) in enumerate(zip(r1, r2)):   # mates interleaved, single reads in between
        recs += [bam_record(a, flag=0x4D), bam_record(b, flag=0x8D)]
        if i < len(extra):
            recs.append(bam_record(extra[i]))
    (tmp_path / "bam").mkdir()
    (tmp_path / "bam" / "s.bam").write_bytes(BC.bgzf(BC.inflated(recs, HEAD)))
    d = tmp_path / "raw" / "tax" / "s"
    d.mkdir(parents=True)
    (d / "s.1.fq").write_bytes(R.fq(r1))
    (d / "s.2.fq").write_bytes(R.fq(r2))
    (d / "s.fq").write_bytes(R.fq(extra))
    (tmp_path / "labels.csv").write_text("sample,labels\ns,tax\n")
    run("image", ["bam", "--from-bam", "--bam-pairs", "--labels-csv", "labels.csv", "-i", "int_A", "--write-splits", "-o", "A", "-f",
                  "A.csv"] + COMMON, tmp_path)
    run("image", ["raw", "--from-raw", "-i", "int_B", "--write-splits", "-o", "B", "-f", "B.csv"] + COMMON, tmp_path)
    same_outputs(tmp_path, "A", "B")
    # without the flag the mates are single reads: nothing is merged, another text
    run("image", ["bam", "--from-bam", "--labels-csv", "labels.csv", "-i", "int_C", "-o", "C", "-f", "C.csv"] + COMMON, tmp_path)
    assert gzip.decompress((tmp_path / "int_C" / "clean_reads" / "s.fq.gz").read_bytes()) != \
        gzip.decompress((tmp_path / "int_A" / "clean_reads" / "s.fq.gz").read_bytes())


DEFAULT_MAX = ["-R", "7", "-m", "50K", "-k", "7"]   # (-M at its default of 200M: the read budget is on)


def test_bam_pairs_on_mates_only_equals_r1_r2_files(tmp_path):
    """An unaligned paired BAM: every read is READ1 or READ2, the SINGLE stream is empty and is no file of the sample."""
    r1, r2, _ = R.synth_set(76, 1000, 0)
    r1, r2 = bare(r1), bare(r2)
    recs = [rec for a, b in zip(r1, r2) for rec in (bam_record(a, flag=0x4D), bam_record(b, flag=0x8D))]
    (tmp_path / "bam").mkdir()
    (tmp_path / "bam" / "s.bam").write_bytes(BC.bgzf(BC.inflated(recs, HEAD)))
    d = tmp_path / "raw" / "tax" / "s"
    d.mkdir(parents=True)
    (d / "s.1.fq").write_bytes(R.fq(r1))
    (d / "s.2.fq").write_bytes(R.fq(r2))
    (tmp_path / "labels.csv").write_text("sample,labels\ns,tax\n")
    run("image", ["bam", "--from-bam", "--bam-pairs", "--labels-csv", "labels.csv", "-i", "int_A", "--write-splits", "-o", "A", "-f",
                  "A.csv"] + DEFAULT_MAX, tmp_path)
    run("image", ["raw", "--from-raw", "-i", "int_B", "--write-splits", "-o", "B", "-f", "B.csv"] + DEFAULT_MAX, tmp_path)
    same_outputs(tmp_path, "A", "B")


def test_bam_pairs_on_single_reads_only_equals_one_file(tmp_path):
    """A single-end BAM run with --bam-pairs: the READ1 and READ2 streams are empty."""
    (tmp_path / "bam").mkdir()
    (tmp_path / "bam" / "s1.bam").write_bytes(sample_bam("s1"))
    d = tmp_path / "raw" / LABELS["s1"] / "s1"
    d.mkdir(parents=True)
    (d / "s1.fq").write_bytes(R.fq(READS["s1"]))
    (tmp_path / "labels.csv").write_text("sample,labels\ns1,%s\n" % LABELS["s1"])
    run("image", ["bam", "--from-bam", "--bam-pairs", "--labels-csv", "labels.csv", "-i", "int_A", "--write-splits", "-o", "A", "-f",
                  "A.csv"] + DEFAULT_MAX, tmp_path)
    run("image", ["raw", "--from-raw", "-i", "int_B", "--write-splits", "-o", "B", "-f", "B.csv"] + DEFAULT_MAX, tmp_path)
    same_outputs(tmp_path, "A", "B")


def test_query_from_bam_equals_from_raw(tmp_path):
    import pandas as pd
    model_files(tmp_path)
    (tmp_path / "bam").mkdir()
    (tmp_path / "raw").mkdir()
    for s in READS:
        (tmp_path / "bam" / f"{s}.bam").write_bytes(sample_bam(s))
        (tmp_path / "raw" / f"{s}.fq").write_bytes(R.fq(READS[s]))
    common = ["-l", "m.pt", "--vocab", "vocab.txt", "-k", "7", "-p", "cgr", "-R", "5", "-M", "100K", "-b", "2", "-P"]
    run("query", ["bam", "out_bam", "--from-bam"] + common, tmp_path)
    run("query", ["raw", "out_raw", "--from-raw"] + common, tmp_path)
    a = pd.read_csv(tmp_path / "out_bam" / "predictions.csv", float_precision="round_trip")
    b = pd.read_csv(tmp_path / "out_raw" / "predictions.csv", float_precision="round_trip")
    assert list(a["sample_id"]) == sorted(READS) and set(a["actual_labels"]) == {"query"}
    assert np.isfinite(a[VOCAB].to_numpy()).all()
    pd.testing.assert_frame_equal(a, b, check_exact=True)


def test_a_truncated_bam_fails_its_sample_only(tmp_path, capsys):
    import pandas as pd
    (tmp_path / "bam").mkdir()
    (tmp_path / "bam" / "good.bam").write_bytes(sample_bam("s1"))
    recs = [bam_record(r) for r in READS["s3"][:500]]
    (tmp_path / "bam" / "cut.bam").write_bytes(BC.bgzf(BC.inflated(recs, HEAD, cut=11)))
    (tmp_path / "bam" / "text.bam").write_bytes(BC.bgzf(R.fq(READS["s3"][:50])))   # BGZF, no BAM inside
    crc = bytearray(BC.bgzf(BC.inflated(recs, HEAD)))
    first_member = (crc[16] | (crc[17] << 8)) + 1
    crc[first_member - 8] ^= 0x55                                                  # the first member fails its CRC-32
    (tmp_path / "bam" / "crc.bam").write_bytes(bytes(crc))
    run("image", ["bam", "--from-bam", "-o", "A", "-f", "A.csv"] + COMMON, tmp_path)
    err = capsys.readouterr().err
    assert err.count("CLEAN FAIL:") == 3 and "cut.bam" in err and "text.bam" in err and "crc.bam" in err
    assert "good.bam" not in err
    stats = pd.read_csv(tmp_path / "A.csv").set_index("sample")
    assert stats.loc["cut", "failed_step"] == "clean" and stats.loc["text", "failed_step"] == "clean"
    assert stats.loc["crc", "failed_step"] == "clean"
    assert pd.isna(stats.loc["good", "failed_step"])
    names = {p.name.split("@")[0] for p in (tmp_path / "A").rglob("*.png")}
    assert names == {"good"}
