"""The host emulation of the PNG encoder (tests/emul/png_emul.cpp around csrc/vk_png.h) as a library that the test
modules share: built on first use into tests/emul/ (again when a source is newer), loaded with ctypes.  The sanitizer
build is a program of its own (sanitizer_program) and is never loaded into python."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "png_emul.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("vk_png.h", "vk_deflate.h", "vk_lane.h")]
GUARD = 0xAB

_run = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    """run(imgs [n, side, side], cap=None) -> (return code, the chunks or None, the bytes behind the buffer's capacity,
    the pieces' sizes [n, pieces], the buffer up to its capacity, offsets, lengths); run.bound(side, n); run.pieces(side)"""
    global _run
    if _run is not None:
        return _run
    so = os.path.join(HERE, "emul", "libpng_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emul_png_bound.restype = C.c_uint64
    L.emul_png_bound.argtypes = [C.c_uint32, C.c_uint32]
    L.emul_png_pieces.restype = C.c_uint32
    L.emul_png_pieces.argtypes = [C.c_uint32]
    L.emul_png.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(imgs, cap=None):
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        n, side = imgs.shape[0], imgs.shape[1]
        bound = L.emul_png_bound(side, n)
        cap = bound if cap is None else cap
        out = np.full(bound + 64, GUARD, dtype=np.uint8)
        offs, lens = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        sizes = np.zeros((n, L.emul_png_pieces(side)), dtype=np.uint64)
        rc = L.emul_png(imgs.ctypes.data, n, side, out.ctypes.data, cap, offs.ctypes.data, lens.ctypes.data, sizes.ctypes.data)
        chunks = [out[int(o):int(o + m)].tobytes() for o, m in zip(offs, lens)] if rc == 0 else None
        return rc, chunks, out[cap:], sizes, out[:cap], offs, lens
    run.bound = L.emul_png_bound
    run.pieces = L.emul_png_pieces
    _run = run
    return run


def encode(imgs):
    """The emulation's chunks of images of one side, guard bytes checked."""
    rc, chunks, guard = load()(imgs)[:3]
    assert rc == 0 and (guard == GUARD).all()
    return chunks


def sanitizer_program(directory):
    """The stand-alone program (-DPNG_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "png_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DPNG_EMUL_MAIN", "-I", CSRC, SRC, "-o", exe])
    return exe


def sha(data):
    return hashlib.sha256(data).hexdigest()
