"""Images for the PNG encoder's tests (csrc/vk_png.h: tests/test_png_emulation.py on the host emulation,
tests/test_gpu_png.py on the GPU), seeded, and the checks of one chunk that need no engine."""
import os
import struct
import zlib
from collections import OrderedDict

import numpy as np

PIECE = 65280             # raw bytes of a piece at most
SIDES = (23, 32, 46, 64, 91, 128, 182, 256, 363, 512)   # one piece up to 182; 256: two, cut inside a row; 363: three; 512: five
SMALL = 128               # up to here every kind of content
LEVELS = np.array([0, 36, 73, 109, 146, 182, 255], dtype=np.uint8)
TABLE_ALLOWANCE = 286     # as tests/deflate_cases.py: what sending the code lengths without run-length symbols may cost
FRAMING = 10              # zlib header, the empty stored block behind a piece, padding
TEXT = (["genus:Aus", "species:Aus bus"], 0.0123, 0.01, "cgr")   # write_png's labels, base_sd, threshold, mapping
HERE = os.path.dirname(os.path.abspath(__file__))
DIGESTS = os.path.join(HERE, "golden", "png_sweep_sha256.json")
GOLDEN_IMAGES = os.path.join(HERE, "golden", "image_small.npz")


def raw_len(side):
    return side * (side + 1)


def pieces(side):
    return -(-raw_len(side) // PIECE)


def raw_stream(arr):
    """The text of the image's zlib stream: every row with the filter byte 0 in front."""
    side = arr.shape[0]
    return np.concatenate([np.zeros((side, 1), dtype=np.uint8), arr], axis=1).tobytes()


def levels7(rng, side):
    """7 distinct levels drawn like Poisson(0.6) counts (what a window's image looks like); the rare high levels are
    planted once each in the middle row, so that every side has all seven."""
    img = LEVELS[np.minimum(rng.poisson(0.6, size=(side, side)), 6)]
    img[side // 2, :7] = LEVELS
    return img


def cases():
    """name -> image [side, side] uint8; names are s<side>_<kind>."""
    rng = np.random.default_rng(8_950)
    golden = np.load(GOLDEN_IMAGES)
    c = OrderedDict()
    for side in SIDES:
        def put(kind, arr):
            assert arr.shape == (side, side) and arr.dtype == np.uint8
            c[f"s{side}_{kind}"] = np.ascontiguousarray(arr)
        put("zero", np.zeros((side, side), dtype=np.uint8))
        put("uniform", rng.integers(0, 256, size=(side, side), dtype=np.uint8))
        put("levels7", levels7(rng, side))
        if side <= SMALL:
            put("all255", np.full((side, side), 255, dtype=np.uint8))
            corners = np.zeros((side, side), dtype=np.uint8)
            corners[0, 0], corners[0, -1], corners[-1, 0], corners[-1, -1] = 1, 2, 3, 255
            put("corners", corners)
            put("equal_rows", np.tile(rng.integers(0, 256, size=(1, side), dtype=np.uint8), (side, 1)))
            for name in golden.files:
                if golden[name].shape == (side, side):
                    put("golden_" + name, golden[name])
    # No side gives a last piece of one byte (256: 512 bytes, 363: 1572, 512: 1536): the shortest is 256's.  Its image has
    # coded bytes in the first piece and random ones in the last (a coded piece that is not the last, then a stored last one)
    short = levels7(rng, 256)
    short[254:] = rng.integers(0, 256, size=(2, 256), dtype=np.uint8)
    c["s256_short_last"] = short
    # and the other way round: a stored piece that is not the last, coded ones behind it
    mixed = levels7(rng, 363)
    mixed[:179] = rng.integers(0, 256, size=(179, 363), dtype=np.uint8)
    c["s363_stored_first"] = mixed
    return c


def by_side(named=None):
    """side -> [(name, image)] in cases()' order"""
    out = OrderedDict((s, []) for s in SIDES)
    for name, arr in (named or cases()).items():
        out[arr.shape[0]].append((name, arr))
    return out


def split_chunk(chunk):
    """(data, crc) of one complete IDAT chunk, its framing checked."""
    n, kind = struct.unpack(">I4s", chunk[:8])
    assert kind == b"IDAT" and len(chunk) == n + 12
    return chunk[8:8 + n], struct.unpack(">I", chunk[-4:])[0]


def huffman_only_size(text):
    c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(c.compress(text) + c.flush())


def piece_texts(arr):
    raw = raw_stream(arr)
    return [raw[at:at + PIECE] for at in range(0, len(raw), PIECE)]


def pieces_fit(arr, piece_sizes):
    """every piece is no larger than zlib's Huffman-only block of the same bytes + the table allowance + the framing"""
    return all(int(size) <= huffman_only_size(t) + TABLE_ALLOWANCE + FRAMING for t, size in zip(piece_texts(arr), piece_sizes))


def halves(arr, size):
    """the stream is under half of the Huffman-only block of the image's raw bytes"""
    return 2 * size < huffman_only_size(raw_stream(arr))


def wants_half(name):
    return name.endswith(("_zero", "_all255", "_equal_rows"))


def check_chunk(name, arr, chunk):
    """Every assertion on one chunk that needs no engine and no piece sizes: zlib inflates its data to the raw stream
    (which checks the Adler-32), the CRC is the chunk's, and the size stays within the bound."""
    data, crc = split_chunk(chunk)
    assert zlib.decompress(data) == raw_stream(arr), name
    assert crc == zlib.crc32(chunk[4:-4]), name
    assert data[:2] == b"\x78\x01", name
    side = arr.shape[0]
    assert len(chunk) <= 16 + 2 + raw_len(side) + 9 * pieces(side), name
    if name.endswith("_uniform"):   # stored blocks: 2 + 5 per piece + the text + 4
        assert len(data) == 2 + 5 * pieces(side) + raw_len(side) + 4, name


def digests(encode, named=None):
    """What tests/golden/png_sweep_sha256.json records, from `encode` (images of one side -> chunks): name -> sha256"""
    import hashlib
    out = {}
    for side, items in by_side(named).items():
        for (name, _), chunk in zip(items, encode(np.stack([a for _, a in items]))):
            out[name] = hashlib.sha256(chunk).hexdigest()
    return out


def file_chunks(data):
    """[(type, payload)] of a PNG file, every chunk's CRC checked, consecutive IDATs counted as one."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload)
        if kind == b"IDAT" and out and out[-1][0] == b"IDAT":
            out[-1] = (kind, out[-1][1] + payload)
        else:
            out.append((kind, payload))
        at += 12 + n
    assert at == len(data)
    return out


def same_file_but_idat(mine, pils):
    """The chunk sequence and every payload but IDAT's equal (PIL chooses a filter per row: the raw streams differ, the
    pixels are opens_like's)."""
    a, b = file_chunks(mine), file_chunks(pils)
    assert [k for k, _ in a] == [k for k, _ in b]
    for (kind, x), (_, y) in zip(a, b):
        assert kind == b"IDAT" or x == y, kind


def opens_like(mine, pils):
    """PIL verifies and loads `mine` (bytes of a file): mode L, pixels and .text those of the file `pils`."""
    import io
    from PIL import Image
    Image.open(io.BytesIO(mine)).verify()
    a, b = Image.open(io.BytesIO(mine)), Image.open(io.BytesIO(pils))
    a.load()
    b.load()
    assert a.mode == "L" == b.mode and a.size == b.size
    assert (np.array(a) == np.array(b)).all()
    assert a.text == b.text and list(a.text) == list(b.text)
