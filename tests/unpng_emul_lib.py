"""The host emulation of the PNG decoder's un-filter (tests/emul/unpng_emul.cpp around csrc/vk_unpng.h) as a library that
the test modules share: built on first use into tests/emul/ (again when a source is newer), loaded with ctypes.  The
sanitizer build is a program of its own (sanitizer_program) and is never loaded into python."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "unpng_emul.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("vk_unpng.h", "vk_png.h", "vk_deflate.h", "vk_lane.h")]
GUARD = 0xAB
PAD = 64

_run = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def adler_word(stream):
    """The four bytes behind a zlib stream's data, read as the decoder hands them on: a little-endian u32."""
    return struct.unpack("<I", stream[-4:])[0]


def load():
    """run(raws, side, wants) -> (return code, images [n, side, side], statuses [n], the guard bytes around the images)"""
    global _run
    if _run is not None:
        return _run
    so = os.path.join(HERE, "emul", "libunpng_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emul_unpng_slot.restype = C.c_uint32
    L.emul_unpng_stride.restype = C.c_uint32
    L.emul_unpng.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(raws, side, wants):
        n = len(raws)
        assert all(len(r) == side * (side + 1) for r in raws)
        raw = np.frombuffer(b"".join(raws), dtype=np.uint8)
        want = np.asarray(wants, dtype=np.uint32)
        out = np.full(PAD + n * side * side + PAD, GUARD, dtype=np.uint8)
        status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        rc = L.emul_unpng(raw.ctypes.data, n, side, want.ctypes.data, None, out[PAD:].ctypes.data, status.ctypes.data)
        guard = np.concatenate([out[:PAD], out[PAD + n * side * side:]])
        return rc, out[PAD:PAD + n * side * side].reshape(n, side, side).copy(), status, guard
    run.slot = L.emul_unpng_slot
    run.stride = L.emul_unpng_stride
    _run = run
    return run


def sanitizer_program(directory):
    """The stand-alone program (-DUNPNG_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "unpng_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DUNPNG_EMUL_MAIN", "-I", CSRC, SRC, "-o", exe])
    return exe


def program_input(side, raws, wants):
    """The bytes of a file the program reads."""
    return struct.pack("<II", side, len(raws)) + b"".join(struct.pack("<I", w) + r for r, w in zip(raws, wants))
