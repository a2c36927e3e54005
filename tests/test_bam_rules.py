"""The rule of `--from-bam` without a GPU: tests/bam_ref.py reproduces hand-written FASTQ for hand-made records;
varkoder_amd.bam reads headers (bounded against hostile lengths) and lists a folder; the command line refuses what the
rule refuses, with exit status 2."""
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_cases as BC  # noqa: E402
import bam_ref as BR  # noqa: E402

from varkoder_amd import bam  # noqa: E402
from varkoder_amd.cli import main, parse_args  # noqa: E402


def convert(records, exclude=BR.EXCLUDE_DEFAULT, head=None):
    head = BC.header(BC.HD_UNSORTED) if head is None else head
    data = BC.inflated(records, head)
    first, _ = BR.header_end(data)
    assert first == len(head)
    return BR.convert(data, first, exclude)


def test_forward_read():
    st, texts, counts = convert([BC.record(b"read/1", "ACGTN", [0, 10, 20, 30, 40])])
    assert st == 0 and counts[BR.ALL] == 1
    assert texts[BR.ALL] == b"@read/1\nACGTN\n+\n!+5?I\n"
    assert texts[BR.SINGLE] == texts[BR.ALL] and texts[BR.READ1] == b"" and texts[BR.READ2] == b""


def test_reverse_read_of_odd_length_with_iupac_and_equals():
    # stored: = A C M G R S V T W Y H K D B N A  (17 bases), qualities 0..16; written reversed and complemented
    st, texts, _ = convert([BC.record(b"r", "=ACMGRSVTWYHKDBNA", list(range(17)), flag=0x10, ref_id=-1)])
    assert st == 0
    assert texts[BR.ALL] == b"@r\nTNVHMDRWABSYCKGTN\n+\n10/.-,+*)('&%$#\"!\n"


def test_absent_qualities_are_I():
    st, texts, _ = convert([BC.record(b"q", "ACG", None), BC.record(b"p", "GT", None, flag=0x14)])
    assert st == 0 and texts[BR.ALL] == b"@q\nACG\n+\nIII\n@p\nAC\n+\nII\n"


def test_quality_above_93_is_clamped():
    st, texts, _ = convert([BC.record(b"q", "ACGT", [92, 93, 94, 200])])
    assert st == 0 and texts[BR.ALL] == b"@q\nACGT\n+\n}~~~\n"


def test_no_bases_no_read():
    st, texts, counts = convert([BC.record(b"empty", "", []), BC.record(b"x", "A", [5])])
    assert st == 0 and counts[BR.ALL] == 1 and texts[BR.ALL] == b"@x\nA\n+\n&\n"


def test_secondary_and_supplementary_are_passed_over():
    recs = [BC.record(b"a", "AC", [1, 2], flag=0), BC.record(b"a", "AC", [1, 2], flag=0x100),
            BC.record(b"a", "GG", [1, 2], flag=0x800), BC.record(b"dup", "TT", [3, 3], flag=0x400),
            BC.record(b"qc", "CA", [4, 4], flag=0x200)]
    st, texts, _ = convert(recs)
    assert st == 0 and texts[BR.ALL] == b"@a\nAC\n+\n\"#\n@dup\nTT\n+\n$$\n@qc\nCA\n+\n%%\n"
    st, texts, _ = convert(recs, exclude=0xF00)
    assert st == 0 and texts[BR.ALL] == b"@a\nAC\n+\n\"#\n"


def test_three_streams():
    recs = [BC.record(b"p", "AC", [1, 1], flag=0x4D), BC.record(b"p", "GT", [2, 2], flag=0x8D),
            BC.record(b"s", "TT", [3, 3], flag=4), BC.record(b"odd", "CC", [4, 4], flag=0xC1),
            BC.record(b"unpaired_first", "GA", [5, 5], flag=0x40)]
    st, texts, counts = convert(recs)
    assert st == 0
    assert texts[BR.READ1] == b"@p\nAC\n+\n\"\"\n"
    assert texts[BR.READ2] == b"@p\nGT\n+\n##\n"
    assert texts[BR.SINGLE] == b"@s\nTT\n+\n$$\n@odd\nCC\n+\n%%\n@unpaired_first\nGA\n+\n&&\n"
    assert counts == {BR.ALL: 5, BR.READ1: 1, BR.READ2: 1, BR.SINGLE: 3}


def test_statuses():
    good = BC.record(b"g", "ACGT", [1, 2, 3, 4])
    data = BC.inflated([good, good], BC.header(), cut=3)
    assert BR.convert(data, 12)[0] == BR.TRUNCATED and BR.convert(data, 12)[1][BR.ALL] == b""
    short = struct.pack("<i", 32 + 2 + 2 + 3) + good[4:]
    assert convert([good, short])[0] == BR.BAD_RECORD
    assert convert([BC.record(raw_name=b"", seq="A", qual=[1])])[0] == BR.BAD_RECORD
    assert convert([BC.record(raw_name=b"ab", seq="A", qual=[1])])[0] == BR.BAD_RECORD


# ---- bam.bam_header, bam.bam_files ------------------------------------------------------------------------------------

def write(path, data, member=0xFF00):
    path.write_bytes(BC.bgzf(data, member))
    return path


def test_header_without_references(tmp_path):
    head = BC.header(b"@HD\tVN:1.6\tSO:unsorted\n")
    p = write(tmp_path / "a.bam", head + BC.record(b"r", "A", [1]))
    assert bam.bam_header(p) == (len(head), 0, "unsorted")
    assert bam.bam_header(write(tmp_path / "b.bam", BC.header())) == (12, 0, "unknown")


def test_header_with_three_references(tmp_path):
    head = BC.header(b"@HD\tVN:1.6\tSO:queryname\tGO:none\n@SQ\tSN:chr1\tLN:1000\n", BC.REFS3)
    p = write(tmp_path / "a.bam", head + BC.record(b"r", "A", [1]))
    assert bam.bam_header(p) == (len(head), 3, "queryname")


def test_header_over_several_members(tmp_path):
    head = BC.header(b"@HD\tVN:1.6\tSO:coordinate\n" + b"@CO\t" + b"x" * 5000 + b"\n", BC.REFS3)
    p = write(tmp_path / "a.bam", head + BC.record(b"r", "ACGT", [1, 2, 3, 4]) * 50, member=300)
    assert bam.bam_header(p) == (len(head), 3, "coordinate")
    assert bam.inflated_size(p) == len(head) + 50 * len(BC.record(b"r", "ACGT", [1, 2, 3, 4]))


@pytest.mark.parametrize("which", ("l_text", "n_ref", "l_name", "negative"))
def test_hostile_header_lengths_are_errors(tmp_path, which, monkeypatch):
    if which == "l_text":
        data = b"BAM\x01" + struct.pack("<i", 0x7FFFFFFF) + b"@HD\n"
    elif which == "n_ref":
        data = BC.header(b"@HD\n")[:-4] + struct.pack("<i", 0x7FFFFFFF)
    elif which == "l_name":
        data = BC.header(b"@HD\n")[:-4] + struct.pack("<ii", 1, 0x7FFFFFF0) + b"chr1\0"
    else:
        data = b"BAM\x01" + struct.pack("<i", -5) + b"@HD\n"
    # never an allocation, never a loop over the stated count: zlib may be asked for no more text than the file holds
    import zlib
    real = zlib.decompress

    def bounded(raw, wbits=15, bufsize=16384):
        assert bufsize <= 65536
        return real(raw, wbits=wbits, bufsize=bufsize)
    monkeypatch.setattr(bam.zlib, "decompress", bounded)
    p = write(tmp_path / "h.bam", data + b"\0" * 100)
    import time
    t0 = time.perf_counter()
    with pytest.raises(bam.BamError):
        bam.bam_header(p)
    assert time.perf_counter() - t0 < 1.0


def test_not_bam(tmp_path):
    with pytest.raises(bam.BamError):
        bam.bam_header(write(tmp_path / "a.bam", b"@read\nACGT\n+\nIIII\n"))
    plain = tmp_path / "b.bam"
    plain.write_bytes(b"BAM\x01" + b"\0" * 40)
    with pytest.raises(bam.BamError):
        bam.bam_header(plain)
    with pytest.raises(bam.BamError):
        bam.inflated_size(plain)


def test_bam_files_names_and_duplicates(tmp_path):
    for name in ("b.bam", "a.x.bam", "c.fq", "d.bam.bai", ".bam"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "dir.bam").mkdir()
    files = bam.bam_files(tmp_path)
    assert [f.name for f in files] == ["a.x.bam", "b.bam"]
    assert [bam.sample_of(f) for f in files] == ["a.x", "b"]
    (tmp_path / "b.BAM").write_bytes(b"")
    with pytest.raises(Exception, match="Two BAM files for sample b"):
        bam.bam_files(tmp_path)


def test_plans_and_size_estimate(tmp_path):
    from varkoder_amd import _capi
    assert bam.sample_plan("s.bam") == [("s.bam", _capi.VK_CL_ROLE_UNPAIRED, _capi.VK_BAM_ALL)]
    assert [(r, s) for _, r, s in bam.sample_plan("s.bam", pairs=True)] == [
        (_capi.VK_CL_ROLE_UNPAIRED, _capi.VK_BAM_SINGLE), (_capi.VK_CL_ROLE_R1, _capi.VK_BAM_READ1),
        (_capi.VK_CL_ROLE_R2, _capi.VK_BAM_READ2)]
    data = dict(BC.unit_cases())["bulk"]
    p = write(tmp_path / "s.bam", data)
    text = BR.convert(data, BR.header_end(data)[0], exclude=0)[1][BR.ALL]
    assert len(data) + len(text) <= bam.batch_bytes(p) <= len(data) * 7 // 3 + bam.FASTQ_SLACK


# ---- the command line --------------------------------------------------------------------------------------------------

QUERY = ["query", "IN", "OUT", "-l", "m.pt", "--vocab", "v.txt"]


@pytest.mark.parametrize("argv", (
    ["image", "IN", "--from-bam", "--from-raw"],
    ["image", "IN", "--from-bam", "--from-clean"],
    ["image", "IN", "--from-bam", "--from-fasta"],
    QUERY + ["--from-bam", "--from-raw"],
    QUERY + ["--from-bam", "--from-fasta"],
    QUERY + ["--from-bam", "--images"],
    ["image", "IN", "--bam-pairs"],
    ["image", "IN", "--from-raw", "--bam-pairs"],
    ["image", "IN", "--from-raw", "--bam-exclude", "0xF00"],
    ["image", "IN", "--from-fasta", "--bam-exclude", "0"],
    QUERY + ["--bam-pairs"],
    QUERY + ["--from-raw", "--bam-exclude", "0xF00"],
))
def test_refusals_exit_2(argv):
    with pytest.raises(SystemExit) as e:
        parse_args(argv)
    assert e.value.code == 2


def test_accepted_forms():
    a = parse_args(["image", "IN", "--from-bam"])
    assert a.from_bam and not hasattr(a, "bam_pairs") and not hasattr(a, "bam_exclude")
    a = parse_args(["image", "IN", "--from-bam", "--bam-pairs", "--bam-exclude", "0xF00", "-i", "INT", "--write-splits", "--gpu-gzip",
                    "--detect-adapters", "-m", "50K", "-M", "200K"])
    assert a.bam_pairs and a.bam_exclude == 0xF00 and a.write_splits and a.gpu_gzip
    a = parse_args(QUERY + ["--from-bam", "--bam-exclude", "2304"])
    assert a.from_bam and a.bam_exclude == 0x900
    assert not hasattr(parse_args(["image", "IN", "--from-raw"]), "from_bam")   # (existing parses are unchanged)


@pytest.mark.parametrize("command", ("image", "query"))
def test_bam_pairs_refuses_a_file_sorted_by_coordinate(tmp_path, capsys, command):
    src = tmp_path / "in"
    src.mkdir()
    write(src / "ok.bam", BC.header(BC.HD_UNSORTED))
    write(src / "sorted_one.bam", BC.header(b"@HD\tVN:1.6\tSO:coordinate\n", BC.REFS3))
    argv = ["image", str(src), "-o", str(tmp_path / "out")] if command == "image" else \
        ["query", str(src), str(tmp_path / "out"), "-l", "m.pt", "--vocab", "v.txt"]
    with pytest.raises(SystemExit) as e:
        main(argv + ["--from-bam", "--bam-pairs"])
    assert e.value.code == 2
    assert "sorted_one.bam" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_file_info_reads_a_file_once(tmp_path, monkeypatch):
    """The batcher, the sort-order check and the upload ask for the same file: its header and size are read once, and
    again only when the file changes."""
    head = BC.header(BC.HD_UNSORTED, BC.REFS3)
    p = write(tmp_path / "a.bam", head + BC.record(b"r", "ACGT", [1, 2, 3, 4]))
    calls = []
    real = bam.bam_header
    monkeypatch.setattr(bam, "bam_header", lambda path: calls.append(path) or real(path))
    want = (len(head) + len(BC.record(b"r", "ACGT", [1, 2, 3, 4])), (len(head), 3, "unsorted"))
    assert bam.file_info(p) == want and bam.batch_bytes(p) > 0 and bam.check_pairs([p]) is None and bam.file_info(p) == want
    assert len(calls) == 1
    bad = tmp_path / "b.bam"
    bad.write_bytes(b"not a bam")
    for _ in range(2):
        with pytest.raises(bam.BamError):
            bam.file_info(bad)
    write(p, BC.header(b"@HD\tVN:1.6\tSO:coordinate\n"))
    os.utime(p, ns=(1, 1))
    assert bam.file_info(p)[1] == (len(BC.header(b"@HD\tVN:1.6\tSO:coordinate\n")), 0, "coordinate") and len(calls) == 2
    assert "a.bam" in bam.check_pairs([p])
