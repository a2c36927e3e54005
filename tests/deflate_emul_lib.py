"""The host emulation of the BGZF compressor (tests/emul/deflate_emul.cpp around csrc/vk_deflate.h) as a library that the
test modules share: built on first use into tests/emul/ (again when a source is newer), loaded with ctypes.  The
sanitizer build is a program of its own (sanitizer_program) and is never loaded into python."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "deflate_emul.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("vk_deflate.h", "vk_lane.h")]
GUARD = 0xAB

_run = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    """run(text, cap=None) -> (return code, the file or None, the bytes behind the buffer's capacity); run.bound(n)"""
    global _run
    if _run is not None:
        return _run
    so = os.path.join(HERE, "emul", "libdeflate_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emul_deflate_bound.restype = C.c_uint64
    L.emul_deflate_bound.argtypes = [C.c_uint64]
    L.emul_deflate.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]

    def run(text, cap=None):
        bound = L.emul_deflate_bound(len(text))
        cap = bound if cap is None else cap
        out = np.full(bound + 64, GUARD, dtype=np.uint8)
        n = C.c_uint64()
        rc = L.emul_deflate(text, len(text), out.ctypes.data, cap, C.byref(n))
        return rc, out[:n.value].tobytes() if rc == 0 else None, out[cap:]
    run.bound = L.emul_deflate_bound
    _run = run
    return run


def compress(text):
    """The emulation's file of one text, guard bytes checked."""
    rc, data, guard = load()(text)
    assert rc == 0 and (guard == GUARD).all()
    return data


def sanitizer_program(directory):
    """The stand-alone program (-DDEFLATE_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "deflate_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DDEFLATE_EMUL_MAIN", "-I", CSRC, SRC, "-o", exe])
    return exe


def sha(data):
    return hashlib.sha256(data).hexdigest()
