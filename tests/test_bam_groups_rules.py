"""`--from-bam --bam-read-groups` without a GPU: the reference converter (tests/bam_groups_ref.py) on hand-written
expectations, bam.read_groups / group_names / group_samples / sample_plan with their errors, the workspace bound of
vk_bam_groups_workspace_size (a file of 1 GiB with 1024 groups x 3 classes stays under the file's own size) and what the
command line refuses."""
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_cases as BC  # noqa: E402
import bam_groups_cases as GC  # noqa: E402
import bam_groups_ref as GR  # noqa: E402
import bam_ref as BR  # noqa: E402

from varkoder_amd import _capi, bam, cli  # noqa: E402

U = GR.UNGROUPED


def one(aux, ids=(b"a", b"bb"), flag=4):
    """The reference on a file of one read `r` (ACGT, qualities 1..4) with this aux area: (status, {key: text})."""
    head = GC.rg_header(list(ids))
    data = head + BC.record(b"r", "ACGT", [1, 2, 3, 4], flag=flag, aux=aux)
    return GR.convert(data, len(head), list(ids))


TEXT = b"@r\nACGT\n+\n\"#$%\n"


def test_reference_on_hand_written_reads():
    assert one(GC.rg(b"bb")) == (0, {(BR.ALL, 1): TEXT, (BR.SINGLE, 1): TEXT})
    assert one(GC.rg(b"a"), flag=0x4D) == (0, {(BR.ALL, 0): TEXT, (BR.READ1, 0): TEXT})
    assert one(b"") == (0, {(BR.ALL, U): TEXT, (BR.SINGLE, U): TEXT})
    for value in (b"", b"b", b"bbb", b"c", b"A"):
        assert set(one(GC.rg(value))[1]) == {(BR.ALL, U), (BR.SINGLE, U)}, value
    assert set(one(b"RGAa" + GC.rg(b"a"))[1]) == {(BR.ALL, U), (BR.SINGLE, U)}          # the first RG decides
    assert set(one(b"RGi" + struct.pack("<i", 1))[1]) == {(BR.ALL, U), (BR.SINGLE, U)}
    assert set(one(BC.aux_z(b"XX", b"RGZa") + GC.rg(b"bb"))[1]) == {(BR.ALL, 1), (BR.SINGLE, 1)}
    assert set(one(b"XBBs" + struct.pack("<I", 2) + b"RGZa" + GC.rg(b"bb"))[1]) == {(BR.ALL, 1), (BR.SINGLE, 1)}
    assert set(one(GC.rg(b"a") + b"junk")[1]) == {(BR.ALL, 0), (BR.SINGLE, 0)}          # nothing behind it is looked at
    assert one(GC.rg(b"a"), flag=0x104) == (0, {})                                      # excluded: no read
    for bad in (b"XXq", b"XXq1", b"XBBq" + struct.pack("<I", 0), b"XBBi" + struct.pack("<I", 2) + b"1234", b"X", b"XC",
                b"Xii123", b"XBBc\x01\0\0"):
        assert one(bad + GC.rg(b"a")) == (GR.BAD_AUX, {}), bad
    assert one(b"XZZabc") == (GR.BAD_AUX, {}) and one(b"XHH1A") == (GR.BAD_AUX, {})     # no NUL in the block
    assert one(b"XXq", flag=0x104) == (0, {})                                           # bad aux of a record that is no read
    head = GC.rg_header([b"a"])
    cut = head + BC.record(b"r", "ACGT", [1, 2, 3, 4], aux=b"XXq")
    assert GR.convert(cut[:-1], len(head), [b"a"])[0] == BR.TRUNCATED                  # the framing's status comes first


def test_reference_keeps_file_order_within_a_text():
    head = GC.rg_header([b"x", b"y"])
    recs = [BC.record(b"r%d" % i, "AC", [5, 6], aux=GC.rg(b"xy"[i % 2:i % 2 + 1])) for i in range(6)]
    status, texts = GR.convert(head + b"".join(recs), len(head), [b"x", b"y"])
    assert status == 0
    assert [line for line in texts[(BR.ALL, 0)].split(b"\n") if line.startswith(b"@")] == [b"@r0", b"@r2", b"@r4"]
    assert [line for line in texts[(BR.ALL, 1)].split(b"\n") if line.startswith(b"@")] == [b"@r1", b"@r3", b"@r5"]


def write(path, data, member=0xFF00):
    path.write_bytes(BC.bgzf(data, member))
    return path


def test_read_groups_and_their_errors(tmp_path):
    ids = [b"run_model_barcode01", b"run_model_barcode02", b"lib 3"]
    p = write(tmp_path / "a.bam", GC.rg_header(ids, BC.REFS3), member=100)
    assert bam.read_groups(p) == ids and bam.read_groups(p) == ids
    assert bam.bam_header(p)[:2] == BR.header_end(GC.rg_header(ids, BC.REFS3))
    assert bam.read_groups(write(tmp_path / "none.bam", BC.header(BC.HD_UNSORTED))) == []
    text = BC.HD_UNSORTED + b"@RG\tSM:x\tID:late\r\n@CO\t@RG\tID:comment\n@RG\tID:second\tID:ignored\n@RGX\tID:no\n"
    assert bam.read_groups(write(tmp_path / "fields.bam", BC.header(text))) == [b"late", b"second"]
    for name, text in (("dup", b"@RG\tID:a\n@RG\tID:b\n@RG\tID:a\n"), ("noid", b"@RG\tID:a\n@RG\tSM:s\n"), ("empty", b"@RG\tID:\tSM:s\n"),
                       ("long", b"@RG\tID:" + b"i" * 256 + b"\n"),
                       ("many", b"".join(b"@RG\tID:%d\n" % i for i in range(1025)))):
        with pytest.raises(bam.BamError):
            bam.read_groups(write(tmp_path / f"{name}.bam", BC.header(text)))
    assert len(bam.read_groups(write(tmp_path / "full.bam", BC.header(b"".join(b"@RG\tID:%d\n" % i for i in range(1024)))))) == 1024
    assert bam.read_groups(write(tmp_path / "255.bam", BC.header(b"@RG\tID:" + b"i" * 255 + b"\n"))) == [b"i" * 255]
    with pytest.raises(bam.BamError):
        bam.read_groups(write(tmp_path / "text.bam", b"not a bam"))


def test_group_names_and_sample_plans(tmp_path):
    assert bam.group_names("s", [b"run7_sup@v5_barcode01", b"a b", b"x" * 150]) == ["s__run7_sup_v5_barcode01", "s__a_b", "s__" + "x" * 100]
    with pytest.raises(bam.BamError):
        bam.group_names("s", [b"a b", b"a_b"])
    with pytest.raises(bam.BamError):
        bam.group_names("s", [b"y" * 100 + b"1", b"y" * 100 + b"2"])
    assert bam.sample_plan("f.bam") == [("f.bam", _capi.VK_CL_ROLE_UNPAIRED, _capi.VK_BAM_ALL)]
    assert bam.sample_plan("f.bam", group=2) == [("f.bam", _capi.VK_CL_ROLE_UNPAIRED, _capi.VK_BAM_ALL, 2)]
    assert bam.sample_plan("f.bam", True, 0) == [("f.bam", _capi.VK_CL_ROLE_UNPAIRED, _capi.VK_BAM_SINGLE, 0),
                                                 ("f.bam", _capi.VK_CL_ROLE_R1, _capi.VK_BAM_READ1, 0),
                                                 ("f.bam", _capi.VK_CL_ROLE_R2, _capi.VK_BAM_READ2, 0)]
    a = write(tmp_path / "a.bam", GC.rg_header([b"g1", b"g2"]))
    plain = write(tmp_path / "plain.bam", BC.header(BC.HD_UNSORTED))
    broken = write(tmp_path / "broken.bam", BC.header(b"@RG\tID:x\n@RG\tID:x\n"))
    members, why = bam.group_samples([a, broken, plain])
    assert members == [("a__g1", a, 0), ("a__g2", a, 1)]
    assert set(why) == {broken, plain} and "twice" in why[broken] and "no @RG" in why[plain]
    clash = write(tmp_path / "a__g2.bam", BC.header(BC.HD_UNSORTED))
    with pytest.raises(Exception, match="Two BAM files for sample a__g2"):
        bam.group_samples([a, clash])


def test_raw_plans_keep_a_files_groups_together():
    """The samples of one file make one plan: one upload, one batch, one rank."""
    from varkoder_amd.pipeline import _raw_plans
    samples = [("a__x", ["a.bam"]), ("a__y", ["a.bam"]), ("b__x", ["b.bam"])]
    opt = {"pairs": True, "exclude": 0x900, "groups": {"a__x": 0, "a__y": 1, "b__x": 0}}
    plans = _raw_plans(samples, [5, 5, 3], 0, 1, opt)
    assert [name for name, _ in plans] == ["a.bam", "b.bam"]
    assert [(e[2], e[3], e[4]) for e in plans[0][1]] == [(sel, g, s) for s, g in (("a__x", 0), ("a__y", 1))
                                                        for sel in (_capi.VK_BAM_SINGLE, _capi.VK_BAM_READ1, _capi.VK_BAM_READ2)]
    shares = [_raw_plans(samples, [5, 5, 3], r, 2, opt) for r in range(2)]
    assert sorted(name for share in shares for name, _ in share) == ["a.bam", "b.bam"] and all(len(s) == 1 for s in shares)


def test_workspace_stays_under_the_file(tmp_path):
    """Condition 2: 1 GiB, 1024 groups x 3 classes (and the ungrouped reads' three streams), the default segments and
    panels -- and the formula of include/vkimg.h, piece by piece."""
    from varkoder_amd.engine import bam_groups_workspace_size
    ids = [b"run7_sup@v5_barcode%04d" % i for i in range(1024)]
    nstreams = 3 * 1025
    got = bam_groups_workspace_size([1 << 30], [ids], [0] * nstreams)
    assert got < (1 << 30) // 3   # (under the file's own size, by a factor of three)

    def up(n):
        return -(-n // 256) * 256
    segs, panels, slots = (1 << 30) // 65536, (1 << 30) // 65536 // 4, 2048
    want = (up(sum(map(len, ids))) + up(4 * 2) + up(4 * 1025) + up(4 * slots) + 2 * up(4) + up(4 * 2) + 3 * up(4 * nstreams)
            + up(2 * 3 * 1025) + up(8 * 2) + up(8) + 2 * up(8 * nstreams)
            + up(4) + up(8) + up(2 * (65536 // 37 + 2) * segs) + up(16 * panels * nstreams) + up(16 * nstreams))
    assert got == want
    small = bam_groups_workspace_size([5000, 0], [ids[:3], []], [0, 0, 1], seg_bytes=256, panel_segs=3)
    assert small < 64 * 1024
    for bad in (dict(seg_bytes=63), dict(seg_bytes=65537), dict(panel_segs=4097)):
        with pytest.raises(_capi.VkError):
            bam_groups_workspace_size([5000], [ids[:3]], [0], **bad)
    with pytest.raises(_capi.VkError):
        bam_groups_workspace_size([5000], [ids[:3]], [1])


def test_the_parser_refuses(tmp_path, capsys):
    (tmp_path / "in").mkdir()
    for argv in (["image", "in", "--bam-read-groups"], ["image", "in", "--from-raw", "--bam-read-groups"],
                 ["query", "in", "out", "--bam-read-groups", "-l", "m.pt", "--vocab", "v.txt"],
                 ["query", "in", "out", "--from-raw", "--bam-read-groups", "-l", "m.pt", "--vocab", "v.txt"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args([str(tmp_path / a) if a == "in" else a for a in argv])
        assert e.value.code == 2
        assert "--bam-read-groups: only with --from-bam" in capsys.readouterr().err
    args = cli.parse_args(["image", str(tmp_path / "in"), "--from-bam", "--bam-read-groups", "--bam-pairs", "--bam-exclude", "0xF00"])
    assert cli.bam_options(args) == {"pairs": True, "exclude": 0xF00, "groups": {}}
    args = cli.parse_args(["image", str(tmp_path / "in"), "--from-bam"])
    assert cli.bam_options(args) == {"pairs": False, "exclude": 0x900, "groups": None}
    args = cli.parse_args(["query", str(tmp_path / "in"), "out", "--from-bam", "--bam-read-groups", "-l", "m.pt", "--vocab", "v.txt"])
    assert cli.bam_options(args)["groups"] == {}
