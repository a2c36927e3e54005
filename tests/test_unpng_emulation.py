"""The PNG decoder's un-filter and Adler-32 function (csrc/vk_unpng.h: unpng_image) compiled for the host
(tests/emul/unpng_emul.cpp), the lanes run one after another, over the files of tests/unpng_cases.py.  PIL is the judge;
the raw stream is zlib's.  No GPU needed.

This covers the ARITHMETIC of unpng_image only: barriers, the LDS atomic, the inflate kernel and the C entry points run in
tests/test_gpu_unpng.py alone."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import unpng_cases as U
import unpng_emul_lib as EM

BAD_ADLER, BAD_FILTER = 8, 16


@pytest.fixture(scope="module")
def emul():
    return EM.load()


@pytest.fixture(scope="module")
def inputs():
    """side -> (names, raw streams, Adler words, pixels)"""
    out = {}
    for side, items in U.by_side().items():
        streams = [U.stream_of(d) for _, d, _ in items]
        out[side] = ([n for n, _, _ in items], [zlib.decompress(s) for s in streams], [EM.adler_word(s) for s in streams],
                     np.stack([a for _, _, a in items]))
    return out


def test_the_layout_constants(emul):
    for side in (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 130, 511, 512):
        s = emul.stride(side)
        assert s >= side + 1 and (s - 1) % 8 == 4, (side, s)   # stride - 1 = 4 * odd: a step's lanes in different banks
        assert emul.slot(side) == (side * (side + 1) + 15) // 16 * 16
    assert emul.stride(512) == 517 and 65 * 517 + 64 + (128 + 4) * 4 <= 64 * 1024


def test_every_case_gives_pils_pixels_with_status_0_and_guards_intact(emul, inputs):
    for side, (names, raws, wants, pixels) in inputs.items():
        rc, img, status, guard = emul(raws, side, wants)
        assert rc == 0 and (guard == EM.GUARD).all(), side
        assert not status.any(), [(n, int(s)) for n, s in zip(names, status) if s]
        wrong = [n for n, a, b in zip(names, img, pixels) if not (a == b).all()]
        assert not wrong, wrong


def test_a_filter_byte_5_and_a_flipped_adler_byte_give_exactly_their_bit(emul, inputs):
    for side in (2, 65, 130):
        names, raws, wants, pixels = inputs[side]
        for row in sorted({0, side - 1, min(64, side - 1)}):
            bad = bytearray(raws[0])
            bad[row * (side + 1)] = 5
            # (the Adler word is the changed stream's: the filter byte alone is wrong)
            word = int.from_bytes(zlib.adler32(bytes(bad)).to_bytes(4, "big"), "little")
            rc, img, status, guard = emul([bytes(bad), raws[1]], side, [word, wants[1]])
            assert rc == 0 and list(status) == [BAD_FILTER, 0] and (guard == EM.GUARD).all(), (side, row)
            assert (img[1] == pixels[1]).all()
        for byte in range(4):
            rc, img, status, guard = emul([raws[0], raws[1]], side, [wants[0] ^ (1 << (8 * byte)), wants[1]])
            assert rc == 0 and list(status) == [BAD_ADLER, 0] and (guard == EM.GUARD).all(), (side, byte)
            assert (img[1] == pixels[1]).all()


def test_the_emulation_under_address_and_undefined_sanitizers(tmp_path, inputs):
    """A stand-alone program (its own main, never loaded into python) built with the sanitizers, once over every case:
    a file of raw streams per side, every stream staged from a buffer of exactly its slot."""
    exe = EM.sanitizer_program(str(tmp_path))
    paths = []
    for side, (names, raws, wants, pixels) in inputs.items():
        p = os.path.join(tmp_path, f"side{side}")
        with open(p, "wb") as f:
            f.write(EM.program_input(side, raws, wants))
        paths.append(p)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    for p, (side, (names, raws, wants, pixels)) in zip(paths, inputs.items()):
        with open(p + ".img", "rb") as f:
            got = f.read()
        n = len(names)
        assert not np.frombuffer(got[:4 * n], dtype=np.uint32).any(), side
        assert got[4 * n:] == pixels.tobytes(), side
