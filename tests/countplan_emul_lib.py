"""The host build of the count launch's plan rule (tests/emul/countplan_emul.cpp around csrc/vk_countplan.h) as a library:
built on first use into tests/emul/ (again when a source is newer), loaded with ctypes."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "countplan_emul.cpp")
DEPS = [SRC, os.path.join(CSRC, "vk_countplan.h")]
NOT_FORCED = 0xFFFFFFFF

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "emul", "libcountplan_emul.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.countplan_pull.restype = None
    L.countplan_pull.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.countplan_tail_helpers.restype = C.c_uint32
    _lib = L
    return L


def pull_plan(resident, nsamples, parts, forced_helpers=NOT_FORCED):
    """(grid, helpers)"""
    out = (C.c_uint32 * 2)()
    load().countplan_pull(resident, nsamples, parts, forced_helpers, out)
    return out[0], out[1]


def tail_helpers():
    return load().countplan_tail_helpers()
