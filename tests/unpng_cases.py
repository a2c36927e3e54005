"""PNG files for the decoder's tests (csrc/vk_unpng.h: tests/test_unpng_emulation.py on the host emulation,
tests/test_gpu_unpng.py on the GPU), seeded.  The images are png_cases.cases() and, at the sides that matter to the
band scheme (1 and 2: no left, no up; 63, 64, 65: the band seam; 130; 512: eight bands), two or three more each.  Files
are made three ways: by PIL (optimize=True: a filter per row of its choosing), by a small writer here that forces the
filter, the DEFLATE flavour and the IDAT split, and by the --gpu-png encoder's emulation.  The six PNG files under
tests/golden/ are in too."""
import glob
import io
import os
import struct
import zlib
from collections import OrderedDict

import numpy as np

import png_cases as P

HERE = os.path.dirname(os.path.abspath(__file__))
EXTRA_SIDES = (1, 2, 63, 64, 65, 130)
FILTERS = (0, 1, 2, 3, 4, "mix")
FLAVOURS = ("stored", "level1", "level9", "fixed")
SPLITS = ("one", "seven", "in_header", "in_adler")
SIGNATURE = b"\x89PNG\r\n\x1a\n"

_files = None


def filtered(arr, mode):
    """The raw stream of the image with filter `mode` on every row ("mix": r % 5)."""
    side = arr.shape[0]
    x = arr.astype(np.int64)
    left = np.zeros_like(x)
    left[:, 1:] = x[:, :-1]
    up = np.zeros_like(x)
    up[1:] = x[:-1]
    ul = np.zeros_like(x)
    ul[1:, 1:] = x[:-1, :-1]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    pred = [np.zeros_like(x), left, up, (left + up) >> 1, paeth]
    kinds = np.array([r % 5 if mode == "mix" else mode for r in range(side)])
    rows = np.stack([(x[r] - pred[kinds[r]][r]) & 255 for r in range(side)]).astype(np.uint8)
    return np.concatenate([kinds.astype(np.uint8)[:, None], rows], axis=1).tobytes()


def deflated(raw, flavour):
    """A zlib stream of `raw`: stored blocks (level 0), level 1, level 9, or fixed codes only (Z_FIXED)."""
    level, strategy = {"stored": (0, zlib.Z_DEFAULT_STRATEGY), "level1": (1, zlib.Z_DEFAULT_STRATEGY),
                       "level9": (9, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED)}[flavour]
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(raw) + c.flush()


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def ihdr(width, height, depth=8, colour=0, compression=0, method=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, compression, method, interlace))


def cuts(stream, split):
    """The IDAT payloads of a stream: one chunk, 7-byte chunks, or two with the cut inside the zlib header / the Adler-32."""
    if split == "one":
        return [stream]
    if split == "seven":
        return [stream[i:i + 7] for i in range(0, len(stream), 7)]
    at = 1 if split == "in_header" else len(stream) - 2
    return [stream[:at], stream[at:]]


def write(side, stream, split="one"):
    """The bytes of an 8-bit greyscale file of side x side around a zlib stream."""
    return SIGNATURE + ihdr(side, side) + b"".join(chunk(b"IDAT", c) for c in cuts(stream, split)) + chunk(b"IEND", b"")


def forced(arr, mode, flavour, split="one"):
    return write(arr.shape[0], deflated(filtered(arr, mode), flavour), split)


def pil_file(arr):
    buf = io.BytesIO()
    from PIL import Image
    Image.fromarray(arr).save(buf, format="PNG", optimize=True)
    return buf.getvalue()


def stream_of(data):
    """A file's zlib stream: its IDAT payloads joined."""
    return b"".join(p for k, p in P.file_chunks(data) if k == b"IDAT")


def images():
    """name -> image: png_cases' and the extra sides'."""
    rng = np.random.default_rng(950_8)
    c = OrderedDict(P.cases())
    for side in EXTRA_SIDES:
        c[f"s{side}_uniform"] = rng.integers(0, 256, size=(side, side), dtype=np.uint8)
        c[f"s{side}_smooth"] = ((np.add.outer(np.arange(side), 3 * np.arange(side)) // 2 + rng.integers(0, 3, size=(side, side))) & 255).astype(np.uint8)
        if side >= 7:
            c[f"s{side}_levels7"] = P.levels7(rng, side)
    return c


def files():
    """name -> (bytes of the file, its pixels [side, side]); computed once, in a fixed order."""
    global _files
    if _files is not None:
        return _files
    import png_emul_lib as EM
    from PIL import Image
    from varkoder_amd.image import PNG_IEND, png_head
    out = OrderedDict()
    imgs = images()
    for name, arr in imgs.items():
        out[f"{name}/pil"] = (pil_file(arr), arr)
    # the forced writer: every filter x every flavour x every split somewhere on the extra sides, on 512 and on two of png_cases'
    pick = [k for k in imgs if int(k[1:].split("_")[0]) in EXTRA_SIDES] + ["s23_levels7", "s91_uniform", "s256_short_last"]
    for i, name in enumerate(pick):
        arr = imgs[name]
        for m, mode in enumerate(FILTERS):   # (3 i + m, i + m: four images in a row have every flavour and every split of a filter)
            flavour, split = FLAVOURS[(3 * i + m) % 4], SPLITS[(i + m) % 4]
            out[f"{name}/f{mode}_{flavour}_{split}"] = (forced(arr, mode, flavour, split), arr)
    for name, mode, flavour, split in (("s512_zero", 4, "level9", "one"), ("s512_uniform", "mix", "stored", "in_adler"),
                                       ("s512_uniform", 3, "level1", "in_header"), ("s512_levels7", "mix", "fixed", "one"),
                                       ("s512_levels7", 4, "level9", "one"), ("s64_levels7", 4, "stored", "seven"),
                                       ("s65_uniform", 3, "fixed", "seven")):
        out[f"{name}/F{mode}_{flavour}_{split}"] = (forced(imgs[name], mode, flavour, split), imgs[name])
    # the --gpu-png encoder's emulation: filter 0, its own blocks
    for side in (23, 64, 256, 512):
        items = P.by_side()[side][:3]
        for (name, arr), ch in zip(items, EM.encode(np.stack([a for _, a in items]))):
            out[f"{name}/gpu_png"] = (png_head(side, *P.TEXT) + ch + PNG_IEND, arr)
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "*.png"))):
        with open(path, "rb") as f:
            data = f.read()
        out["golden/" + os.path.basename(path)] = (data, np.array(Image.open(io.BytesIO(data))))
    _files = out
    return out


def by_side():
    """side -> [(name, file bytes, pixels)]"""
    out = OrderedDict()
    for name, (data, arr) in files().items():
        out.setdefault(arr.shape[0], []).append((name, data, arr))
    return out
