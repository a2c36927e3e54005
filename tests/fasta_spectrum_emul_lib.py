"""The host emulation of the assemblies' k-mer spectrum (tests/emul/fasta_spectrum_emul.cpp around
csrc/vk_fasta_spectrum.h) as a library: built on first use into tests/emul/ (again when a source is newer), loaded with
ctypes.  The sanitizer build is a program of its own (sanitizer_program) and is never loaded into python."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "fasta_spectrum_emul.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("vk_fasta_spectrum.h", "vk_fasta.h", "vk_screen.h", "vk_spectrum.h")]
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", CSRC]
EMPTY = np.uint64(2 ** 64 - 1)

_run = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    """run(text, k, every, unit, nslots) -> (status, totals = [records, bases, windows, taken windows, additions],
    {key: count} of the held slots)."""
    global _run
    if _run is not None:
        return _run
    so = os.path.join(HERE, "emul", "libfasta_spectrum_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCLUDES + [SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emul_fasta_spectrum.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]

    def run(text, k, every, unit, nslots):
        text = bytes(text)
        keys = np.zeros(nslots, dtype=np.uint64)
        counts = np.zeros(nslots, dtype=np.uint32)
        totals = np.zeros(5, dtype=np.uint64)
        status = np.zeros(1, dtype=np.uint32)
        rc = L.emul_fasta_spectrum(text, len(text), k, every, unit, nslots, keys.ctypes.data, counts.ctypes.data,
                                   totals.ctypes.data, status.ctypes.data)
        assert rc == 0, rc
        held = keys != EMPTY
        return int(status[0]), [int(x) for x in totals], dict(zip(keys[held].tolist(), counts[held].tolist()))
    _run = run
    return run


def sanitizer_program(directory):
    """The stand-alone program (-DFASTA_SPECTRUM_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(str(directory), "fasta_spectrum_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DFASTA_SPECTRUM_EMUL_MAIN"] + INCLUDES + [SRC, "-o", exe])
    return exe


def run_program(exe, directory, samples, unit):
    """samples: (text, k, every, nslots).  Returns per sample (status, totals, {key: count})."""
    src, dst = os.path.join(str(directory), "in.bin"), os.path.join(str(directory), "out.bin")
    with open(src, "wb") as f:
        for text, k, every, nslots in samples:
            f.write(struct.pack("<IIII", k, every, nslots, len(text)) + bytes(text))
    r = subprocess.run([exe, src, dst, str(unit)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    raw = open(dst, "rb").read()
    out, at = [], 0
    for _ in samples:
        status, = struct.unpack_from("<I", raw, at)
        vals = struct.unpack_from("<6Q", raw, at + 4)
        at += 52
        held = vals[5]
        pairs = np.frombuffer(raw, dtype=np.dtype([("k", "<u8"), ("c", "<u4")]), count=held, offset=at)
        at += 12 * held
        out.append((status, list(vals[:5]), dict(zip(pairs["k"].tolist(), pairs["c"].tolist()))))
    assert at == len(raw)
    return out
