"""The decoder's case files and its numpy reference stand on PIL: for every file of tests/unpng_cases.py, the reference's
pixels of zlib's text of the joined IDAT payloads are PIL's.  Everything else about the decoder is judged by these two."""
import io
import zlib

import numpy as np

import unpng_cases as U
from unpng_ref import unpng_ref


def test_the_cases_are_what_the_issue_lists():
    files, sides = U.files(), U.by_side()
    for side in (1, 2, 63, 64, 65, 130, 512) + tuple(U.P.SIDES):
        assert side in sides
    assert len({n.split("/")[0] for n, _, _ in sides[512]}) == 3, "three images of side 512"
    forced = [n.split("/")[1] for n in files if "/f" in n or "/F" in n]
    for mode in U.FILTERS:
        for flavour in U.FLAVOURS:
            assert any(f[1:].startswith(f"{mode}_{flavour}_") for f in forced), (mode, flavour)
    for split in U.SPLITS:
        assert any(f.endswith(split) for f in forced), split
    assert sum(n.startswith("golden/") for n in files) == 6 and sum(n.endswith("/gpu_png") for n in files) >= 10
    assert sum(n.endswith("/pil") for n in files) == len(U.images())
    # the splits are what they say
    data = files["s64_levels7/F4_stored_seven"][0]
    spans = [p for k, p in _chunks(data) if k == b"IDAT"]
    assert len(spans) > 100 and all(len(p) == 7 for p in spans[:-1])
    assert [len(p) for k, p in _chunks(files["s512_uniform/F3_level1_in_header"][0]) if k == b"IDAT"][0] == 1
    assert [len(p) for k, p in _chunks(files["s512_uniform/Fmix_stored_in_adler"][0]) if k == b"IDAT"][1] == 2


def _chunks(data):
    import struct
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        out.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def test_forced_filters_are_in_the_streams():
    files = U.files()
    for name, (data, arr) in files.items():
        tag = name.split("/")[1]
        if tag[0] in "fF" and tag[1] in "01234m":
            side = arr.shape[0]
            kinds = np.frombuffer(zlib.decompress(U.stream_of(data)), dtype=np.uint8).reshape(side, side + 1)[:, 0]
            want = np.arange(side) % 5 if tag[1] == "m" else np.full(side, int(tag[1]))
            assert (kinds == want).all(), name
    # and PIL's own files carry more than one filter type between them
    seen = set()
    for name, (data, arr) in files.items():
        if name.endswith("/pil") and arr.shape[0] >= 23:
            side = arr.shape[0]
            seen |= set(np.frombuffer(zlib.decompress(U.stream_of(data)), dtype=np.uint8).reshape(side, side + 1)[:, 0].tolist())
    assert len(seen) >= 3, seen


def test_the_reference_gives_pils_pixels_on_every_case_file():
    from PIL import Image
    for name, (data, arr) in U.files().items():
        side = arr.shape[0]
        pil = np.array(Image.open(io.BytesIO(data)))
        assert pil.dtype == np.uint8 and (pil == arr).all(), name
        assert (unpng_ref(zlib.decompress(U.stream_of(data)), side) == pil).all(), name
