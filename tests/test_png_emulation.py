"""The PNG encoder's piece function and join (csrc/vk_png.h) compiled for the host (tests/emul/png_emul.cpp), the lanes
run one after another, over the images of tests/png_cases.py.  zlib and PIL are the judges.  No GPU needed.

This covers the ARITHMETIC of vk_png.h only: barriers, LDS atomics, the scans, the gather kernel and the C entry points
run in tests/test_gpu_png.py alone.  What ties the two together is tests/golden/png_sweep_sha256.json: the digest of the
emulation's chunk for every image, checked here against the emulation and there against the GPU's bytes.

The size conditions are the BGZF compressor's (tests/test_gpu_deflate.py): (1) every piece is no larger than zlib's
Huffman-only block of the same bytes + 286 bytes of table allowance + 10 of framing; (2) every all-equal and equal-rows
image is under half of the Huffman-only block of its raw stream.  What zlib level 1 and PIL's own file (optimize=True:
level 9) do with them is asserted below with zlib itself: both meet (2) everywhere and (1) on the uniform, all-equal,
corner and equal-rows images, and both MISS (1) on every 7-level image from side 64 on -- at 128x128 PIL's IDAT is 4,148
bytes, level 1's 4,943, against 3,314 + 296, where the encoder here writes 3,331: greedy matches in Poisson-like
pixels cost more than the literals they replace, which is why the block of the literals alone is priced too."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as P
import png_emul_lib as EM

GUARD = EM.GUARD


@pytest.fixture(scope="module")
def emul():
    return EM.load()


@pytest.fixture(scope="module")
def encoded(emul):
    """side -> [(name, image, chunk, piece sizes)], the guard bytes and the packing checked"""
    out = {}
    for side, items in P.by_side().items():
        rc, chunks, guard, sizes, buf, offs, lens = emul(np.stack([a for _, a in items]))
        assert rc == 0 and (guard == GUARD).all(), side
        assert (offs % 16 == 0).all() and offs[0] == 0
        for i in range(len(items) - 1):
            end = int(offs[i] + lens[i])
            assert end <= offs[i + 1] < end + 16 and not buf[end:int(offs[i + 1])].any()
        out[side] = [(n, a, c, s) for (n, a), c, s in zip(items, chunks, sizes)]
    return out


@pytest.fixture(scope="module")
def pil_files(tmp_path_factory):
    """name -> the bytes of the file write_png writes for the image with P.TEXT"""
    from varkoder_amd.image import write_png
    d = tmp_path_factory.mktemp("pil")
    out = {}
    for name, arr in P.cases().items():
        write_png(arr, d / "x.png", *P.TEXT)
        out[name] = (d / "x.png").read_bytes()
    return out


def test_the_cases_are_what_the_issue_lists():
    c = P.cases()
    assert [P.pieces(s) for s in P.SIDES] == [1, 1, 1, 1, 1, 1, 1, 2, 3, 5]
    assert P.PIECE % 257 != 0 and [P.raw_len(s) % P.PIECE for s in (256, 363, 512)] == [512, 1572, 1536]
    for side in P.SIDES:
        kinds = ["zero", "uniform", "levels7"] + (["all255", "corners", "equal_rows"] if side <= P.SMALL else [])
        assert all(f"s{side}_{k}" in c for k in kinds)
        assert len(np.unique(c[f"s{side}_levels7"])) == 7
    assert sum("golden" in n for n in c) >= 20 and "s256_short_last" in c and "s363_stored_first" in c
    assert all((a == b).all() for a, b in zip(c.values(), P.cases().values())), "seeded"


def test_every_chunk_inflates_to_the_raw_stream_and_carries_its_crc(encoded):
    for items in encoded.values():
        for name, arr, chunk, _ in items:
            P.check_chunk(name, arr, chunk)


def test_the_files_open_with_pil_and_differ_from_its_files_in_idat_alone(encoded, pil_files):
    from varkoder_amd.image import PNG_IEND, png_head
    for side, items in encoded.items():
        head = png_head(side, *P.TEXT)
        for name, arr, chunk, _ in items:
            mine = head + chunk + PNG_IEND
            P.opens_like(mine, pil_files[name])
            P.same_file_but_idat(mine, pil_files[name])
            assert zlib.decompress(dict(P.file_chunks(mine))[b"IDAT"]) == P.raw_stream(arr), name


def test_a_second_run_gives_the_same_bytes_and_a_short_buffer_nothing(emul, encoded):
    for side in (23, 256):
        imgs = np.stack([a for _, a, _, _ in encoded[side]])
        assert emul(imgs)[1] == [c for _, _, c, _ in encoded[side]]
        rc, chunks, guard = emul(imgs, cap=emul.bound(side, len(imgs)) - 1)[:3]
        assert rc == 6 and chunks is None and (guard == GUARD).all()
    assert [emul.bound(s, 1) for s in (23, 128, 256, 512)] == [592, 16544, 65840, 262720]
    assert emul.bound(128, 100000) == 100000 * 16544


def test_every_piece_is_within_huffman_only_and_the_allowance(encoded):
    for items in encoded.values():
        for name, arr, _, sizes in items:
            assert P.pieces_fit(arr, sizes), (name, list(sizes), [P.huffman_only_size(t) for t in P.piece_texts(arr)])


def test_mixed_images_hold_stored_and_coded_pieces(encoded):
    by = {n: (a, s) for items in encoded.values() for n, a, _, s in items}
    arr, sizes = by["s256_short_last"]
    assert sizes[0] < 20000 and sizes[1] == 512 + 5
    arr, sizes = by["s363_stored_first"]
    assert sizes[0] == 2 + 5 + P.PIECE and sizes[1] < 20000 and sizes[2] < 1000


@pytest.mark.parametrize("side", [s for s in P.SIDES])
def test_equal_images_are_under_half_of_huffman_only(encoded, side):
    """Condition (2).  At side 23 the first round of 256 positions is 10 of the 23 rows, and the hash table only knows
    earlier rounds: the condition is met through the candidate one row back (all255 17 bytes against 85 / 2, equal_rows
    38 against 349 / 2; without that candidate 56 and 215)."""
    for name, arr, chunk, _ in encoded[side]:
        if P.wants_half(name):
            size = len(P.split_chunk(chunk)[0])
            print(name, size, P.huffman_only_size(P.raw_stream(arr)))
            assert P.halves(arr, size), (name, size, P.huffman_only_size(P.raw_stream(arr)))


def test_what_zlib_level_1_and_pil_do_with_the_size_conditions(pil_files):
    """The figures of the module docstring, from zlib itself on the same inputs."""
    def level1(text):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        return len(c.compress(text) + c.flush())
    for name, arr in P.cases().items():
        side = arr.shape[0]
        kind = name.split("_", 1)[1]
        if kind.startswith("golden"):
            continue
        texts = P.piece_texts(arr)
        allowed = [P.huffman_only_size(t) + P.TABLE_ALLOWANCE + P.FRAMING for t in texts]
        zlib_meets = all(level1(t) + P.FRAMING <= a for t, a in zip(texts, allowed))
        pil_idat = len(dict(P.file_chunks(pil_files[name]))[b"IDAT"])
        pil_meets = pil_idat <= sum(allowed)
        misses = kind in ("short_last", "stored_first") or (kind == "levels7" and side >= 64)
        assert zlib_meets == pil_meets == (not misses), (name, pil_idat, sum(allowed))
        if P.wants_half(name):
            assert P.halves(arr, level1(P.raw_stream(arr))) and P.halves(arr, pil_idat), name
    arr = P.cases()["s128_levels7"]
    assert len(dict(P.file_chunks(pil_files["s128_levels7"]))[b"IDAT"]) > P.huffman_only_size(P.raw_stream(arr)) + 296


def test_the_recorded_digests_are_the_emulations(encoded):
    """tests/golden/png_sweep_sha256.json is what the GPU's bytes are compared with (tests/test_gpu_png.py, on a machine
    that needs no compiler for it): it must be the emulation's output of today, entry by entry."""
    with open(P.DIGESTS) as f:
        recorded = json.load(f)
    assert recorded == {n: EM.sha(c) for items in encoded.values() for n, _, c, _ in items}


def test_the_emulation_under_address_and_undefined_sanitizers(tmp_path, encoded):
    """A stand-alone program (its own main, never loaded into python) built with the sanitizers, once over the cases: a
    file of images per side, in a buffer of exactly their size."""
    exe = EM.sanitizer_program(str(tmp_path))
    paths = []
    for side, items in encoded.items():
        p = os.path.join(tmp_path, f"side{side}")
        with open(p, "wb") as f:
            f.write(np.uint32(side).tobytes() + b"".join(a.tobytes() for _, a, _, _ in items))
        paths.append(p)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    for p, items in zip(paths, encoded.values()):
        with open(p + ".idat", "rb") as f:
            assert f.read() == b"".join(c for _, _, c, _ in items)
