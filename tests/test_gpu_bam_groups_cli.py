"""`image --from-bam --bam-read-groups` and `query --from-bam --bam-read-groups` end to end on the GPU.  The input is a folder
with one BAM of three read groups -- one of them without reads -- plus reads of no listed group, and a second, plain BAM
without @RG lines.  The run gives the PNGs `<file>__<id>@...`, their stats.csv rows and the stderr line on the reads passed
over; the images, rows and predictions equal those of `--from-bam` on the same reads written by the test as one BAM per
group (what `samtools split` would have made); once also with --bam-pairs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_cases as BC  # noqa: E402
import bam_groups_cases as GC  # noqa: E402
import clean_ref as R  # noqa: E402
from test_gpu_bam_cli import bam_record, bare, run  # noqa: E402
from test_gpu_query_raw import VOCAB, model_files  # noqa: E402

pytestmark = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "50K", "-M", "200K", "-k", "5", "-t"]
# the header lists the empty group last: the samples' rows (seeds go by row) are then those of the per-group files
IDS = [b"run1_sup@v5_barcode01", b"run1_sup@v5_barcode02", b"run1_sup@v5_barcode03"]
NAMES = ["multi__run1_sup_v5_barcode01", "multi__run1_sup_v5_barcode02"]
HEAD = GC.rg_header(IDS, BC.REFS3)
PLAIN = BC.header(BC.HD_UNSORTED, BC.REFS3)


def single_sets():
    return [bare(R.synth_set(81, 0, 1500)[2]), bare(R.synth_set(82, 0, 1300)[2])], bare(R.synth_set(83, 0, 200)[2])


def write_single(tmp):
    """multi.bam: the reads of two groups interleaved (every fifth of group 2 stored from the reverse strand, secondary
    copies in between), every seventh record a read of no listed group (no RG, or an RG the header does not list);
    plain.bam: reads, no @RG line.  sep/: one BAM per group of the same reads in the same order.  Returns the reads
    passed over."""
    groups, loose = single_sets()
    recs, sep, passed = [], [[], []], 0
    for i in range(max(map(len, groups))):
        for g in range(2):
            if i < len(groups[g]):
                kw = dict(flag=0, reverse=True, ref_id=1, pos=i, cigar=(len(groups[g][i][1]) << 4,)) if g == 1 and i % 5 == 0 else {}
                recs.append(bam_record(groups[g][i], aux=b"NMC\x01" + GC.rg(IDS[g]), **kw))
                sep[g].append(bam_record(groups[g][i], **kw))
                if i % 6 == 0:
                    recs.append(bam_record(groups[g][i], flag=0x100, aux=GC.rg(IDS[g])))
        if i % 7 == 0 and i // 7 < len(loose):
            recs.append(bam_record(loose[i // 7], aux=GC.rg(b"run1_sup@v5_unclassified") if i % 2 else b""))
            passed += 1
    (tmp / "in").mkdir()
    (tmp / "sep").mkdir()
    (tmp / "in" / "multi.bam").write_bytes(BC.bgzf(BC.inflated(recs, HEAD)))
    (tmp / "in" / "plain.bam").write_bytes(BC.bgzf(BC.inflated([bam_record(r) for r in loose], PLAIN)))
    for name, own in zip(NAMES, sep):
        (tmp / "sep" / f"{name}.bam").write_bytes(BC.bgzf(BC.inflated(own, PLAIN)))
    (tmp / "labels_in.csv").write_text("sample,labels\nmulti,taxA\n%s,taxB\n" % NAMES[1])
    (tmp / "labels_sep.csv").write_text("sample,labels\n%s,taxA\n%s,taxB\n" % tuple(NAMES))
    return passed


def same_images_and_rows(tmp, a, b):
    import pandas as pd
    pa = {p.name: p for p in (tmp / a).rglob("*.png")}
    pb = {p.name: p for p in (tmp / b).rglob("*.png")}
    assert pa and sorted(pa) == sorted(pb)
    for name in pa:
        assert pa[name].read_bytes() == pb[name].read_bytes(), name
    assert {n.split("@")[0] for n in pa} == set(NAMES)
    sa, sb = pd.read_csv(tmp / f"{a}.csv"), pd.read_csv(tmp / f"{b}.csv")
    keep = [c for c in sa.columns if not c.endswith("_time")]
    assert list(sa["sample"]) == NAMES and "clean_basepairs" in keep
    pd.testing.assert_frame_equal(sa[keep], sb[keep], check_exact=True)
    la, lb = pd.read_csv(tmp / a / "labels.csv"), pd.read_csv(tmp / b / "labels.csv")
    pd.testing.assert_frame_equal(la, lb)
    assert list(la["labels"]) == ["taxA", "taxB"]   # (the file's label for group 1, its own for group 2)


def test_image_by_read_group_equals_one_bam_per_group(tmp_path, capsys):
    passed = write_single(tmp_path)
    run("image", ["in", "--from-bam", "--bam-read-groups", "--labels-csv", "labels_in.csv", "-o", "A", "-f", "A.csv", "-v"] + COMMON,
        tmp_path)
    err = capsys.readouterr().err
    assert f"multi.bam: {passed} reads without a listed read group passed over" in err
    assert "plain.bam: no @RG line" in err
    assert "multi__run1_sup_v5_barcode03 has no reads" in err
    assert "CLEAN FAIL" not in err
    run("image", ["sep", "--from-bam", "--labels-csv", "labels_sep.csv", "-o", "B", "-f", "B.csv"] + COMMON, tmp_path)
    same_images_and_rows(tmp_path, "A", "B")


def test_image_by_read_group_with_bam_pairs(tmp_path, capsys):
    """Mates of two groups interleaved, a few single reads of group 1, mates without RG: R1 / R2 / single texts per group."""
    sets = [R.synth_set(84, 700, 0), R.synth_set(85, 600, 0)]
    extra = bare(R.synth_set(86, 0, 150)[2])
    loose = R.synth_set(87, 40, 0)
    recs, sep = [], [[], []]
    for i in range(700):
        for g, (r1, r2, _) in enumerate(sets):
            if i < len(r1):
                a, b = bare(r1)[i], bare(r2)[i]
                recs += [bam_record(a, flag=0x4D, aux=GC.rg(IDS[g])), bam_record(b, flag=0x8D, aux=GC.rg(IDS[g]))]
                sep[g] += [bam_record(a, flag=0x4D), bam_record(b, flag=0x8D)]
        if i < len(extra):
            recs.append(bam_record(extra[i], aux=GC.rg(IDS[0])))
            sep[0].append(bam_record(extra[i]))
        if i < 40:
            recs += [bam_record(bare(loose[0])[i], flag=0x4D), bam_record(bare(loose[1])[i], flag=0x8D, aux=GC.rg(b"other"))]
    (tmp_path / "in").mkdir()
    (tmp_path / "sep").mkdir()
    (tmp_path / "in" / "multi.bam").write_bytes(BC.bgzf(BC.inflated(recs, HEAD)))
    for name, own in zip(NAMES, sep):
        (tmp_path / "sep" / f"{name}.bam").write_bytes(BC.bgzf(BC.inflated(own, PLAIN)))
    (tmp_path / "labels_in.csv").write_text("sample,labels\nmulti,taxA\n%s,taxB\n" % NAMES[1])
    (tmp_path / "labels_sep.csv").write_text("sample,labels\n%s,taxA\n%s,taxB\n" % tuple(NAMES))
    run("image", ["in", "--from-bam", "--bam-read-groups", "--bam-pairs", "--labels-csv", "labels_in.csv", "-o", "A", "-f", "A.csv"] + COMMON,
        tmp_path)
    assert "multi.bam: 80 reads without a listed read group passed over" in capsys.readouterr().err
    run("image", ["sep", "--from-bam", "--bam-pairs", "--labels-csv", "labels_sep.csv", "-o", "B", "-f", "B.csv"] + COMMON, tmp_path)
    same_images_and_rows(tmp_path, "A", "B")


def test_query_by_read_group_equals_one_bam_per_group(tmp_path, capsys):
    import pandas as pd
    passed = write_single(tmp_path)
    model_files(tmp_path)
    common = ["-l", "m.pt", "--vocab", "vocab.txt", "-k", "5", "-p", "cgr", "-R", "5", "-M", "100K", "-b", "2", "-P"]
    run("query", ["in", "out_groups", "--from-bam", "--bam-read-groups"] + common, tmp_path)
    assert f"multi.bam: {passed} reads without a listed read group passed over" in capsys.readouterr().err
    run("query", ["sep", "out_sep", "--from-bam"] + common, tmp_path)
    a = pd.read_csv(tmp_path / "out_groups" / "predictions.csv", float_precision="round_trip")
    b = pd.read_csv(tmp_path / "out_sep" / "predictions.csv", float_precision="round_trip")
    assert list(a["sample_id"]) == NAMES and set(a["actual_labels"]) == {"query"}
    assert np.isfinite(a[VOCAB].to_numpy()).all()
    pd.testing.assert_frame_equal(a, b, check_exact=True)
