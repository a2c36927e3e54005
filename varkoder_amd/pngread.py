"""--gpu-png-read: the image files of `train` and `query --images` decoded on the GPU (vk_unpng_device).

A file is ELIGIBLE when it is what `image` writes: 8-bit greyscale, square, at most 512 pixels a side, not interlaced,
one zlib stream with a 32 KiB window at most and no preset dictionary.  Its stream (the IDAT payloads joined in file
order) is laid out in one pinned buffer with the streams of the other files and decoded where the pixels are wanted.
Every other file, and every file the decoder reports a status for, is decoded by PIL exactly as without the flag:
the flag never changes a result, only where the work is done."""
import io
import struct
import zlib
from collections import namedtuple

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 512
ALIGN = 16          # every stream starts at a multiple of this
TAIL = 4            # side * (side + 1) as a little-endian u32 behind the stream's Adler-32 (include/vkimg.h)
SLACK = 1024        # bytes behind the last stream of a call's buffer

Parts = namedtuple("Parts", "width height depth colour compression method interlace spans head length")
Parts.__doc__ = """IHDR's fields; spans: [(start, end)] of the IDAT payloads in the file's bytes, in file order; head: the
first two bytes of the joined stream; length: the joined stream's bytes."""


def png_parts(data):
    """The Parts of a file's bytes, or None when the bytes are not a chunk sequence from the signature to IEND with an
    IHDR of 13 bytes in front, or when the CRC-32 of IHDR or of an IDAT chunk is not its bytes' (PIL refuses those)."""
    if data[:8] != SIGNATURE:
        return None
    at, n = 8, len(data)
    fields, spans = None, []
    while at + 12 <= n:
        size, kind = struct.unpack_from(">I4s", data, at)
        end = at + 8 + size
        if end + 4 > n:
            return None
        if fields is None:
            if kind != b"IHDR" or size != 13:
                return None
            if zlib.crc32(data[at + 4:end]) != struct.unpack_from(">I", data, end)[0]:
                return None
            fields = struct.unpack_from(">IIBBBBB", data, at + 8)
        elif kind == b"IDAT":
            if zlib.crc32(data[at + 4:end]) != struct.unpack_from(">I", data, end)[0]:
                return None
            if size:
                spans.append((at + 8, end))
        elif kind == b"IEND":
            head = b""
            for a, b in spans:   # (the header may be cut into one-byte chunks)
                head += bytes(data[a:min(b, a + 2 - len(head))])
                if len(head) == 2:
                    break
            return Parts(*fields, spans, head, sum(b - a for a, b in spans))
        at = end + 4
    return None


def eligible(parts):
    """True when vk_unpng_device can take the file: see the module's docstring."""
    if parts is None or parts.width != parts.height or not 0 < parts.width <= MAX_SIDE:
        return False
    if (parts.depth, parts.colour, parts.compression, parts.method, parts.interlace) != (8, 0, 0, 0, 0):
        return False
    if parts.length < 2 + 4 or len(parts.head) != 2:
        return False
    cmf, flg = parts.head
    return (cmf & 15) == 8 and (cmf >> 4) <= 7 and not (flg & 32) and (cmf * 256 + flg) % 31 == 0


def stream_layout(lengths):
    """offsets (multiples of ALIGN), lengths with the TAIL, and the bytes of the buffer for streams of `lengths` bytes"""
    lens = np.asarray(lengths, dtype=np.uint64) + np.uint64(TAIL)
    rounded = (lens + np.uint64(ALIGN - 1)) // np.uint64(ALIGN) * np.uint64(ALIGN)
    offs = np.zeros(len(lens), dtype=np.uint64)
    if len(lens) > 1:
        offs[1:] = np.cumsum(rounded[:-1])
    return offs, lens, int(rounded.sum()) + SLACK


def pack_streams(datas, parts, side, out=None):
    """The streams of the files `datas` (their Parts: `parts`) in one buffer as vk_unpng_device reads them: stream i at
    offs[i], a multiple of 16, its bytes, then side * (side + 1) as four bytes little-endian.  -> (buffer, offs, lens);
    out: a uint8 array of at least the layout's bytes to fill instead of a new one."""
    offs, lens, total = stream_layout([p.length for p in parts])
    buf = np.zeros(total, dtype=np.uint8) if out is None else out
    tail = np.frombuffer(struct.pack("<I", side * (side + 1)), dtype=np.uint8)
    for data, p, o in zip(datas, parts, offs):
        at = int(o)
        view = memoryview(data)
        for a, b in p.spans:
            buf[at:at + b - a] = np.frombuffer(view[a:b], dtype=np.uint8)
            at += b - a
        buf[at:at + TAIL] = tail
    return buf, offs, lens


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


def pil_array(path):
    """What both commands do without the flag."""
    from PIL import Image
    return np.array(Image.open(path))


def read_images(engine, paths, pool=None, datas=None, mixed="Images of different sizes are not supported."):
    """The images of the files `paths` as one device tensor, what torch.from_numpy(np.stack([np.array(Image.open(p)) for
    p in paths])).to(engine.device) gives: eligible files through engine.unpng, the others and those with a status
    through PIL (whose exceptions are raised).  pool: an executor to read the files with; datas: their bytes when the
    caller has read them already.  Files of more than one shape: Exception(mixed), before anything is decoded on the
    GPU."""
    import torch
    paths = list(paths)
    if datas is None:
        datas = list(pool.map(read_file, paths)) if pool is not None else [read_file(p) for p in paths]
    parts = [png_parts(d) for d in datas]
    on_gpu = [i for i, p in enumerate(parts) if eligible(p)]
    by_pil = {i: pil_array(paths[i]) for i in range(len(paths)) if not eligible(parts[i])}
    shapes = {(parts[i].height, parts[i].width) for i in on_gpu} | {a.shape for a in by_pil.values()}
    if len(shapes) > 1:
        raise Exception(mixed)
    if not on_gpu or any(a.dtype != np.uint8 for a in by_pil.values()):   # nothing for the decoder, or not bytes: PIL's route whole
        arrays = [by_pil[i] if i in by_pil else pil_array(paths[i]) for i in range(len(paths))]
        return torch.from_numpy(np.stack(arrays)).to(engine.device)
    side = parts[on_gpu[0]].width
    sel = [parts[i] for i in on_gpu]
    offs, lens, total = stream_layout([p.length for p in sel])
    pinned = torch.empty(total, dtype=torch.uint8).pin_memory()
    pinned[total - SLACK:] = 0
    pack_streams([datas[i] for i in on_gpu], sel, side, out=pinned.numpy())
    decoded, status = engine.unpng((pinned, offs, lens), side)
    for i, st in zip(on_gpu, status):
        if st:
            by_pil[i] = pil_array(paths[i])   # raises what PIL raises for a damaged file
    if not by_pil:
        return decoded
    images = torch.empty((len(paths), side, side), dtype=torch.uint8, device=engine.device)
    images[torch.tensor(on_gpu, device=engine.device)] = decoded
    rows = sorted(by_pil)
    images[torch.tensor(rows, device=engine.device)] = torch.from_numpy(np.stack([by_pil[i] for i in rows])).to(engine.device)
    return images
