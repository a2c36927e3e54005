"""The BGZF compressor's member kernel (csrc/vk_deflate.h) compiled for the host (tests/emul/deflate_emul.cpp), its
lanes run one after another, over the texts of tests/deflate_cases.py with the assertions of the GPU test.  zlib is the
judge.  No GPU needed.

This covers the ARITHMETIC of vk_deflate.h only: barriers, LDS atomics, the gather kernel and the C entry points run in
tests/test_gpu_deflate.py alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deflate_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "deflate_emul.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("vk_deflate.h", "vk_lane.h")]
GUARD = 0xAB


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(HERE, "emul", "libdeflate_emul.so")
    if _stale(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", so])
    L = C.CDLL(so)
    L.emul_deflate_bound.restype = C.c_uint64
    L.emul_deflate_bound.argtypes = [C.c_uint64]
    L.emul_deflate.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]

    def run(text, cap=None):
        """(return code, the file, the bytes behind the buffer's capacity)"""
        bound = L.emul_deflate_bound(len(text))
        cap = bound if cap is None else cap
        out = np.full(bound + 64, GUARD, dtype=np.uint8)
        n = C.c_uint64()
        rc = L.emul_deflate(text, len(text), out.ctypes.data, cap, C.byref(n))
        return rc, out[:n.value].tobytes() if rc == 0 else None, out[cap:]
    run.bound = L.emul_deflate_bound
    return run


@pytest.fixture(scope="module")
def files(emul):
    named = list(D.texts().items()) + [(f"small_{i}", t) for i, t in enumerate(D.small_files())]
    out = []
    for name, text in named:
        rc, data, guard = emul(text)
        assert rc == 0 and (guard == GUARD).all(), name
        out.append((name, text, data))
    return out


def test_every_file_inflates_to_its_text_and_is_bgzf(files):
    from varkoder_amd import engine as E
    for name, text, data in files:
        D.check_file(name, text, data)
        assert E.bgzf_members(data) is not None and E.bgzf_text_size(data) == len(text), name


def test_a_second_run_gives_the_same_bytes(emul, files):
    for name, text, data in files[:40]:
        assert emul(text)[1] == data, name


def test_bound_and_a_buffer_one_byte_short(emul):
    assert [emul.bound(n) for n in (0, 1, 65280, 65281)] == [32, 64, 65344, 65376]
    for n in (0, 1, 65280, 65281, 200000):
        assert emul.bound(n) == (D.bound(n) + 15) // 16 * 16
    text = D.texts()["fastq_long_header"]
    rc, data, guard = emul(text, cap=emul.bound(len(text)) - 1)
    assert rc == 6 and data is None and (guard == GUARD).all()


def test_what_zlib_level_1_itself_does_with_the_size_checks():
    """The figures quoted in tests/test_gpu_deflate.py's docstring: level 1 meets both conditions on the FASTQ-shaped
    texts and the repeated record, and misses the first on the skewed text."""
    import zlib
    for name, text in D.texts().items():
        if not (name.startswith("fastq_") or name in ("skewed", "repeated")):
            continue
        for at in range(0, len(text), D.MEMBER):
            t = text[at:at + D.MEMBER]
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            size = len(c.compress(t) + c.flush()) + D.FRAMING
            ok = size <= D.huffman_only_size(t) + D.TABLE_ALLOWANCE + D.FRAMING
            assert ok == (name != "skewed"), (name, size, D.huffman_only_size(t))
            if name == "repeated":
                assert 2 * size < D.huffman_only_size(t)


def test_the_emulation_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program (its own main, never loaded into python) built with the sanitizers, once over the list."""
    exe = os.path.join(tmp_path, "deflate_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DDEFLATE_EMUL_MAIN", "-I", CSRC, SRC, "-o", exe])
    named = list(D.texts().items()) + [(f"small_{i}", t) for i, t in enumerate(D.small_files()[:30])]
    paths = []
    for name, text in named:
        p = os.path.join(tmp_path, name)
        with open(p, "wb") as f:
            f.write(text)
        paths.append(p)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    for (name, text), p in zip(named, paths):
        with open(p + ".gz", "rb") as f:
            D.check_file(name, text, f.read())
