"""The host emulation of the lane-local device code of adapters by sequence (tests/emul/adapter_emul.cpp around
csrc/vk_adapter.h) as a library: built on first use into tests/emul/ (again when a source is newer), loaded with
ctypes.  The sanitizer build is a program of its own (sanitizer_program) and is never loaded into python."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "adapter_emul.cpp")
STUB = os.path.join(HERE, "emul", "stub")
DEPS = [SRC, os.path.join(CSRC, "vk_adapter.h")]
INCLUDES = ["-I", STUB, "-I", CSRC]
NKEYS = 4 ** 10
TOP = 10

_lib = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "emul", "libadapter_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCLUDES + [SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.emul_trim_seq.restype = C.c_uint32
    L.emul_trim_seq.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
    L.emul_key_ok.argtypes = [C.c_void_p]
    L.emul_hist.argtypes = [C.c_char_p, C.c_uint64, u64p, C.c_uint32, C.c_void_p]
    L.emul_collect.argtypes = [C.c_char_p, C.c_uint64, u64p, C.c_uint32, u32p, u32p, C.c_uint32, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]
    _lib = L
    return L


def trim_seq(read, adapter):
    """cl_trim_seq's new length of the read."""
    return load().emul_trim_seq(read, len(read), adapter, len(adapter))


def key_ok():
    ok = np.zeros(NKEYS, dtype=np.uint8)
    load().emul_key_ok(ok.ctypes.data)
    return ok.astype(bool)


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def hist(text, group_n):
    """uint32[groups, 4^10] of vk_ad_hist_kernel: group k is the next group_n[k] records of the text."""
    n = np.ascontiguousarray(group_n, dtype=np.uint64)
    out = np.empty((len(n), NKEYS), dtype=np.uint32)
    rc = load().emul_hist(text, len(text), _u64(n), len(n), out.ctypes.data)
    assert rc == 0, rc
    return out


def collect(text, group_n, keys, caps, shift_tail):
    """(counts uint32[groups, 10], [[(at, fwd, back)] per candidate] per group) of vk_ad_collect_kernel for the
    candidates keys / caps [groups, 10] (cap 0: none)."""
    n = np.ascontiguousarray(group_n, dtype=np.uint64)
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    caps = np.ascontiguousarray(caps, dtype=np.uint32)
    assert keys.shape == caps.shape == (len(n), TOP)
    nocc = int(caps.sum())
    counts = np.empty((len(n), TOP), dtype=np.uint32)
    at = np.empty(nocc + 1, dtype=np.uint64)
    fwd = np.empty(nocc + 1, dtype=np.uint32)
    back = np.empty(nocc + 1, dtype=np.uint32)
    rc = load().emul_collect(text, len(text), _u64(n), len(n), _u32(keys), _u32(caps), shift_tail, counts.ctypes.data,
                             at.ctypes.data, fwd.ctypes.data, back.ctypes.data)
    assert rc == 0, rc
    off = np.concatenate([[0], np.cumsum(caps.ravel())]).astype(np.int64)
    lists = []
    for k in range(len(n)):
        row = []
        for c in range(TOP):
            i = k * TOP + c
            m = min(int(counts[k, c]), int(caps[k, c]))
            row.append([(int(at[off[i] + x]), int(fwd[off[i] + x]), int(back[off[i] + x])) for x in range(m)])
        lists.append(row)
    return counts, lists


def sanitizer_program(directory):
    """The stand-alone program (-DADAPTER_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "adapter_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DADAPTER_EMUL_MAIN"] + INCLUDES + [SRC, "-o", exe])
    return exe
