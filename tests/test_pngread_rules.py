"""--gpu-png-read on the host (varkoder_amd/pngread.py): what png_parts finds in a file against PIL, which files are
eligible for the GPU decoder, how the streams are laid out for vk_unpng_device, the parser's rules for the flag and
vk_unpng_workspace_size.  No GPU needed."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest

import png_cases as P
import unpng_cases as U
from varkoder_amd import _capi, cli, pngread as R


def patched_ihdr(data, **fields):
    """The file with IHDR fields changed and IHDR's CRC made right again."""
    names = ["width", "height", "depth", "colour", "compression", "method", "interlace"]
    values = list(struct.unpack_from(">IIBBBBB", data, 16))
    for k, v in fields.items():
        values[names.index(k)] = v
    return data[:8] + U.chunk(b"IHDR", struct.pack(">IIBBBBB", *values)) + data[33:]


def restreamed(data, change):
    """The file with its zlib stream replaced by change(stream), in one IDAT chunk with a right CRC."""
    p = R.png_parts(data)
    stream = change(bytearray(b"".join(data[a:b] for a, b in p.spans)))
    return data[:p.spans[0][0] - 8] + U.chunk(b"IDAT", bytes(stream)) + U.chunk(b"IEND", b"")


def test_png_parts_finds_pils_size_and_mode_and_the_spans_of_split_idats():
    from PIL import Image
    for name, (data, arr) in U.files().items():
        p = R.png_parts(data)
        im = Image.open(io.BytesIO(data))
        assert (p.width, p.height) == im.size and im.mode == "L" and (p.depth, p.colour) == (8, 0), name
        joined = b"".join(data[a:b] for a, b in p.spans)
        assert joined == U.stream_of(data) and p.length == len(joined) and p.head == joined[:2], name
        assert R.eligible(p), name
        tag = name.split("/")[1]
        if tag.endswith("seven"):
            assert len(p.spans) == -(-len(joined) // 7) and all(b - a == 7 for a, b in p.spans[:-1]), name
        if tag.endswith("in_header"):
            assert [b - a for a, b in p.spans] == [1, len(joined) - 1], name
        if tag.endswith("in_adler"):
            assert [b - a for a, b in p.spans] == [len(joined) - 2, 2], name


def with_fdict(s):
    """The stream with FDICT set in a header whose check bits are right."""
    flg = (s[1] & 0xC0) | 32
    flg += (31 - (s[0] * 256 + flg) % 31) % 31
    return bytes([s[0], flg]) + s[2:]


def test_idats_that_are_not_consecutive_are_joined_in_file_order_and_text_chunks_stay_pils(tmp_path):
    from PIL import Image
    from varkoder_amd.image import write_png
    arr = P.cases()["s46_levels7"]
    write_png(arr, tmp_path / "x.png", *P.TEXT)
    data = (tmp_path / "x.png").read_bytes()
    p = R.png_parts(data)
    assert R.eligible(p) and len(p.spans) == 1
    assert Image.open(io.BytesIO(data)).info == Image.open(tmp_path / "x.png").info and "varkoderKeywords" in Image.open(io.BytesIO(data)).info
    stream = data[p.spans[0][0]:p.spans[0][1]]
    at = p.spans[0][0] - 8
    apart = data[:at] + U.chunk(b"IDAT", stream[:9]) + U.chunk(b"tEXt", b"k\0v") + U.chunk(b"IDAT", stream[9:]) + U.chunk(b"IEND", b"")
    q = R.png_parts(apart)
    assert len(q.spans) == 2 and b"".join(apart[a:b] for a, b in q.spans) == stream


def test_what_is_not_a_sound_chunk_sequence_has_no_parts():
    data = U.files()["s23_levels7/pil"][0]
    assert R.png_parts(b"") is None and R.png_parts(b"GIF89a" + data) is None and R.png_parts(data[:40]) is None
    assert R.png_parts(data[:-12]) is None, "no IEND"
    p = R.png_parts(data)
    flipped = bytearray(data)
    flipped[p.spans[0][0] + 5] ^= 1   # a byte of the stream: the chunk's CRC is wrong now, PIL refuses the file
    assert R.png_parts(bytes(flipped)) is None and not R.eligible(None)
    wrong_ihdr = bytearray(data)
    wrong_ihdr[16 + 3] ^= 1
    assert R.png_parts(bytes(wrong_ihdr)) is None


def test_eligible_is_false_for_what_the_decoder_does_not_take():
    from PIL import Image
    rng = np.random.default_rng(5)
    data = U.files()["s23_levels7/pil"][0]
    assert R.eligible(R.png_parts(data))

    def pil(im, **kw):
        buf = io.BytesIO()
        im.save(buf, format="PNG", **kw)
        return buf.getvalue()
    not_taken = {
        "rgb": pil(Image.fromarray(rng.integers(0, 256, size=(23, 23, 3), dtype=np.uint8))),
        "16_bit": pil(Image.fromarray(rng.integers(0, 65536, size=(23, 23), dtype=np.uint16))),
        "palette": pil(Image.fromarray(rng.integers(0, 256, size=(23, 23), dtype=np.uint8)).convert("P")),
        "not_square": pil(Image.fromarray(rng.integers(0, 256, size=(23, 24), dtype=np.uint8))),
        "side_513": pil(Image.fromarray(np.zeros((513, 513), dtype=np.uint8))),
        "patched_rgb": patched_ihdr(data, colour=2),
        "patched_16_bit": patched_ihdr(data, depth=16),
        "patched_palette": patched_ihdr(data, colour=3),
        "patched_not_square": patched_ihdr(data, width=24),
        "patched_side_513": patched_ihdr(data, width=513, height=513),
        "interlace_1": patched_ihdr(data, interlace=1),
        "compression_1": patched_ihdr(data, compression=1),
        "filter_method_1": patched_ihdr(data, method=1),
        "side_0": patched_ihdr(data, width=0, height=0),
        "fdict": restreamed(data, with_fdict),
        "cm_9": restreamed(data, lambda s: bytes([(s[0] & 0xF0) | 9]) + s[1:]),
        "cinfo_8": restreamed(data, lambda s: bytes([0x88, 0x1C]) + s[2:]),
        "fcheck": restreamed(data, lambda s: s[:1] + bytes([s[1] ^ 1]) + s[2:]),
        "five_bytes": restreamed(data, lambda s: s[:5]),
        "no_idat": data[:33] + U.chunk(b"IEND", b""),
    }
    for name, bad in not_taken.items():
        p = R.png_parts(bad)
        assert p is not None and not R.eligible(p), name
    fd = R.png_parts(not_taken["fdict"]).head
    assert fd[1] & 32 and (fd[0] * 256 + fd[1]) % 31 == 0, "FDICT set in a header that is sound otherwise"
    assert (0x88 * 256 + 0x1C) % 31 == 0
    assert R.eligible(R.png_parts(pil(Image.fromarray(np.zeros((512, 512), dtype=np.uint8)))))
    assert R.eligible(R.png_parts(restreamed(data, lambda s: s)))


def test_the_stream_layout_is_the_headers():
    """include/vkimg.h: every stream at a multiple of 16, from its zlib header to its Adler-32, then side * (side + 1) as
    a little-endian u32; lengths count those four bytes."""
    items = U.by_side()[65][:9]
    datas, parts = [d for _, d, _ in items], [R.png_parts(d) for _, d, _ in items]
    buf, offs, lens = R.pack_streams(datas, parts, 65)
    assert offs[0] == 0 and (offs % 16 == 0).all() and buf.dtype == np.uint8
    ends = offs + lens
    assert (ends[:-1] <= offs[1:]).all() and (offs[1:] - ends[:-1] < 16).all(), "packed, not overlapping"
    assert len(buf) >= int(ends[-1]) + R.SLACK
    for d, o, n in zip(datas, offs, lens):
        stream = U.stream_of(d)
        assert int(n) == len(stream) + 4
        assert buf[int(o):int(o) + len(stream)].tobytes() == stream
        assert buf[int(o) + len(stream):int(o + n)].tobytes() == struct.pack("<I", 65 * 66)
        assert zlib.decompressobj().decompress(buf[int(o):int(o + n)].tobytes()) == zlib.decompress(stream)
    header = open(R.__file__.replace("varkoder_amd/pngread.py", "include/vkimg.h")).read()
    assert "multiples of 16" in header and "little-endian u32" in header and "VK_UNPNG_BAD_FILTER 16u" in header


def test_the_flag_is_long_form_only_absent_when_not_given_and_refused_without_images(capsys):
    q = ["query", "in", "out", "-l", "m", "--vocab", "v"]
    assert cli.parse_args(q + ["-I", "--gpu-png-read"]).gpu_png_read
    assert cli.parse_args(["train", "in", "out", "--gpu-png-read"]).gpu_png_read
    assert not hasattr(cli.parse_args(q + ["-I"]), "gpu_png_read") and not hasattr(cli.parse_args(["train", "in", "out"]), "gpu_png_read")
    for argv, said in ((q + ["--gpu-png-read"], "--gpu-png-read: only with -I/--images"),
                       (q + ["--from-fasta", "--gpu-png-read"], "--gpu-png-read: only with -I/--images"),
                       (q + ["-I", "-m", "--gpu-png"], "--gpu-png: not with -I/--images"),
                       (["image", "in", "--gpu-png-read"], "unrecognized arguments"),
                       (["convert", "--gpu-png-read", "cgr", "in", "out"], "unrecognized arguments")):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
        assert said in capsys.readouterr().err, argv
    for cmd in ("train", "query"):
        with pytest.raises(SystemExit):
            cli.parse_args([cmd, "--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert "--gpu-png-read" in text and "decoded by PIL as without the flag" in text
        assert not any(short + ", --gpu-png-read" in text for short in "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")


def test_the_workspace_is_a_slot_per_image_and_tables():
    L = _capi.lib()
    ws = C.c_uint64(7)
    for side, n in ((0, 1), (513, 1), (128, 0)):
        assert L.vk_unpng_workspace_size(side, n, C.byref(ws)) == _capi.VK_EINVAL and ws.value == 7
    assert L.vk_unpng_workspace_size(128, 1, None) == _capi.VK_EINVAL
    for side in (1, 65, 512):
        slot = (side * (side + 1) + 15) // 16 * 16
        assert L.vk_unpng_workspace_size(side, 1000, C.byref(ws)) == _capi.VK_OK
        assert 1000 * slot <= ws.value <= 1000 * (slot + 64) + 4096, side
