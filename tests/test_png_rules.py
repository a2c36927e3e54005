"""--gpu-png on the host: the file around the IDAT chunk (image.png_head, PNG_IEND, write_png_parts) against write_png's
file chunk by chunk, the parser's rules for the flag, what the product's own readers make of a file in the GPU's format
(the chunk from the host emulation of csrc/vk_png.h), and vk_png_bound.  No GPU needed."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest

import png_cases as P
import png_emul_lib as EM
from varkoder_amd import _capi, cli
from varkoder_amd.image import PNG_IEND, png_head, write_png, write_png_parts

LABELS = (["genus:Aus", "species:Aus bus"], ["λ-clade;Ωmega", "plain"], [])


def host_idat(arr):
    """A complete IDAT chunk made by the host's zlib: filter byte 0 in front of every row."""
    data = zlib.compress(P.raw_stream(arr), 6)
    return struct.pack(">I", len(data)) + b"IDAT" + data + struct.pack(">I", zlib.crc32(b"IDAT" + data))


@pytest.mark.parametrize("labels", LABELS, ids=["latin", "not_latin_1", "none"])
@pytest.mark.parametrize("base_sd", [0, 0.0123])
def test_head_parts_and_iend_against_write_png(tmp_path, labels, base_sd):
    arr = P.cases()["s46_levels7"]
    text = (labels, base_sd, 0.01, "varKode")
    write_png(arr, tmp_path / "pil.png", *text)
    write_png_parts(tmp_path / "parts.png", png_head(46, *text), host_idat(arr))
    mine, pils = (tmp_path / "parts.png").read_bytes(), (tmp_path / "pil.png").read_bytes()
    P.same_file_but_idat(mine, pils)
    P.opens_like(mine, pils)
    kinds = [k for k, _ in P.file_chunks(mine)]
    assert kinds == [b"IHDR", kinds[1], b"tEXt", b"tEXt", b"tEXt", b"IDAT", b"IEND"]
    assert kinds[1] == (b"iTXt" if labels == LABELS[1] else b"tEXt")
    assert mine.endswith(PNG_IEND) and PNG_IEND == bytes.fromhex("0000000049454e44ae426082")
    from PIL import Image
    im = Image.open(io.BytesIO(mine))
    assert im.text["varkoderKeywords"] == ";".join(labels) and im.text["varkoderLowQualityFlag"] == str(base_sd > 0.01)


def test_the_flag_is_long_form_only_absent_when_not_given_and_refused_twice(capsys):
    q = ["query", "in", "out", "-l", "m", "--vocab", "v"]
    assert cli.parse_args(["image", "in", "--gpu-png"]).gpu_png
    assert cli.parse_args(["image", "in", "--from-fasta", "--windows", "--gpu-png"]).gpu_png
    assert cli.parse_args(["image", "in", "--from-raw", "-i", "int", "--gpu-gzip", "--gpu-png"]).gpu_png
    assert cli.parse_args(q + ["-m", "--gpu-png"]).gpu_png
    assert cli.parse_args(q + ["--from-fasta", "--keep-images", "--gpu-png"]).gpu_png
    assert not hasattr(cli.parse_args(["image", "in"]), "gpu_png") and not hasattr(cli.parse_args(q + ["-m"]), "gpu_png")
    for argv, said in ((q + ["--gpu-png"], "--gpu-png: only with -m/--keep-images"),
                       (["image", "in", "--from-raw", "-i", "int", "--write-splits", "-X", "--gpu-png"], "--gpu-png: not with -X/--no-image"),
                       (["convert", "--gpu-png", "cgr", "in", "out"], "unrecognized arguments")):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
        assert said in capsys.readouterr().err
    parser_help = []
    for cmd in ("image", "query"):
        with pytest.raises(SystemExit):
            cli.parse_args([cmd, "--help"])
        parser_help.append(" ".join(capsys.readouterr().out.split()))
    for text in parser_help:
        assert "--gpu-png" in text and "pixels and text chunks are the same" in text and "bytes are not" in text
        assert not any(short + ", --gpu-png" in text for short in "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")


def test_the_products_readers_read_a_file_in_the_gpu_format_as_they_read_pils(tmp_path):
    """query --images' loader (PIL, the name's metadata, image_metadata of the text chunks, the array) and train's
    input listing (collect_images) on two folders: the same images written by write_png and in the GPU's format."""
    from PIL import Image
    from varkoder_amd.convert import get_metadata_from_img_filename
    from varkoder_amd.query import image_metadata
    from varkoder_amd.train import collect_images
    named = [("sampleA@00010000K+cgr+k7.png", P.cases()["s128_levels7"], (["genus:Aus", "species:Aus bus"], 0.02, 0.01, "cgr")),
             ("sampleB@00000500K+varKode+k7.png", P.cases()["s91_levels7"], (["λ-clade"], 0.001, 0.01, "varKode"))]
    for folder in ("pil", "gpu"):
        (tmp_path / folder).mkdir()
    for name, arr, text in named:
        write_png(arr, tmp_path / "pil" / name, *text)
        write_png_parts(tmp_path / "gpu" / name, png_head(arr.shape[0], *text), EM.encode(arr[None])[0])

    def loaded(p):
        im = Image.open(p)
        md = get_metadata_from_img_filename(p)
        md.pop("path")
        return md, image_metadata(im.info), np.array(im)
    for name, arr, _ in named:
        a, b = loaded(tmp_path / "gpu" / name), loaded(tmp_path / "pil" / name)
        assert a[0] == b[0] and a[1] == b[1] and (a[2] == b[2]).all() and (a[2] == arr).all() and a[2].dtype == np.uint8
    a, b = collect_images(tmp_path / "gpu"), collect_images(tmp_path / "pil")
    assert a.drop(columns="path").equals(b.drop(columns="path")) and len(a) == 2
    assert list(a["labels"]) == ["genus:Aus;species:Aus bus", "λ-clade"]


def test_the_bound_is_the_headers_formula_and_the_emulations():
    L = _capi.lib()
    emul = EM.load()
    for side in P.SIDES:
        for n in (1, 3, 100000):
            b = C.c_uint64()
            assert L.vk_png_bound(side, n, C.byref(b)) == _capi.VK_OK
            per = (16 + 2 + side * (side + 1) + 9 * P.pieces(side) + 15) // 16 * 16
            assert b.value == n * per == emul.bound(side, n)
    b = C.c_uint64(7)
    for side, n in ((0, 1), (513, 1), (128, 0)):
        assert L.vk_png_bound(side, n, C.byref(b)) == _capi.VK_EINVAL and b.value == 7
        assert L.vk_png_workspace_size(side, n, C.byref(b)) == _capi.VK_EINVAL and b.value == 7
    assert L.vk_png_bound(128, 1, None) == _capi.VK_EINVAL
    ws = C.c_uint64()
    assert L.vk_png_workspace_size(128, 100000, C.byref(ws)) == _capi.VK_OK
    assert 100000 * 16528 < ws.value < 100000 * 16700, "a slot is the piece's bound, not 65,536"
