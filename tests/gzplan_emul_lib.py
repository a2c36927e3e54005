"""The host build of the inflate's plans (tests/emul/gzplan_emul.cpp around csrc/vk_gzplan.h) as a library that the tests
share: built on first use into tests/emul/ (again when a source is newer), loaded with ctypes.  The sanitizer build is a
program of its own (sanitizer_program) and is never loaded into python.  A walk, member or direct case is a flat list of
u64 words (walk_case, members_case, direct_case); run() answers through the library, run_program() through a program."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "gzplan_emul.cpp")
DEPS = [SRC, os.path.join(CSRC, "vk_gzplan.h")]
INFLATED, TOO_LARGE, GO_DIRECT = 0, 1, 2   # a verdict's kind
END = 0xFFFFFFFF                           # kGzEnd

_lib = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "emul", "libgzplan_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    u64p = C.POINTER(C.c_uint64)
    for name in ("gzplan_mem_rec", "gzplan_chunk_min", "gzplan_big_file"):
        getattr(L, name).restype = C.c_uint32
    L.gzplan_fit.restype = C.c_uint32
    L.gzplan_fit.argtypes = [u64p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
    L.gzplan_table.restype = C.c_int64
    L.gzplan_table.argtypes = [C.c_uint32, u64p, u64p, u64p, C.c_uint32, u64p, C.c_uint64]
    L.gzplan_crc_zeros.restype = C.c_uint32
    L.gzplan_crc_zeros.argtypes = [C.c_uint64]
    L.gzplan_run.restype = C.c_int64
    L.gzplan_run.argtypes = [u64p, C.c_uint64, u64p, C.c_uint64]
    _lib = L
    return L


def _u64(values):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def fit(lengths, slots, forced=0, fill=0):
    """chunk_bytes of a call whose big files have these compressed lengths."""
    a, p = _u64(lengths)
    return load().gzplan_fit(p, a.size, slots, forced, fill)


def table(chunk_bytes, offsets, lengths, caps):
    """(sym_total, chunk0 per file, chunks as dicts)"""
    (o, po), (n, pn), (c, pc) = _u64(offsets), _u64(lengths), _u64(caps)
    out = np.zeros(1 << 16, dtype=np.uint64)
    got = load().gzplan_table(chunk_bytes, po, pn, pc, o.size, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size)
    assert got >= 0
    w = out[:got].tolist()
    sym_total, nc = w[0], w[1]
    chunk0 = w[2:2 + o.size]
    keys = ("in_off", "in_len", "out_off", "out_cap", "file_chunk0", "nchunks", "chunk_bytes")
    rest = w[2 + o.size:]
    assert len(rest) == 7 * nc
    return sym_total, chunk0, [dict(zip(keys, rest[7 * i:7 * i + 7])) for i in range(nc)]


def walk_case(files, chunks):
    """files: [(text_off, cap, number of chunks)]; chunks: one dict per chunk of the call, in order, with the keys sym_off,
    len, status, next, isize, members ([(end, crc)], what the wavefront has on record) and optionally nmem (the member
    count it reports, where that is not len(members))."""
    R = load().gzplan_mem_rec()
    nc, chunk0, w = len(chunks), [], [1, len(chunks), len(files)]
    c = 0
    for _, _, n in files:
        chunk0.append(c)
        for j in range(n):
            w += [0, n << 17, chunks[c + j]["sym_off"], 1 << 20, c, n, 1 << 17]
        c += n
    assert c == nc
    w += chunk0
    for key in ("len", "status", "next", "isize"):
        w += [ch[key] for ch in chunks]
    w += [ch.get("nmem", len(ch["members"])) for ch in chunks]
    for ch in chunks:
        assert len(ch["members"]) <= R
        for end, crc in ch["members"]:
            w += [end, crc]
        w += [0, 0] * (R - len(ch["members"]))
    w += [f[0] for f in files] + [f[1] for f in files]
    return w


def members_case(file, text_off, text_len, members):
    return [2, file, len(members), text_off, text_len] + [x for m in members for x in m]


def direct_case(file, status, nmem, text_off, text_len, records):
    return [3, file, status, nmem, text_off, text_len, len(records)] + [x for r in records for x in r]


def _checks(w, at):
    n = w[at]
    return [tuple(w[at + 1 + 4 * j:at + 5 + 4 * j]) for j in range(n)], at + 1 + 4 * n   # (text_off, text_len, file, want)


def parse(case, w):
    """The answer to a case as a dict."""
    if case[0] == 1:
        nbig = case[2]
        res = {"verdict": [tuple(w[3 * b:3 * b + 3]) for b in range(nbig)]}   # (kind, status, total)
        at = 3 * nbig
        ni = w[at]
        res["items"] = [tuple(w[at + 1 + 3 * i:at + 4 + 3 * i]) for i in range(ni)]   # (sym_off, len, text_off)
        at += 1 + 3 * ni
        nok = w[at]
        res["ok"] = [tuple(w[at + 1 + 3 * i:at + 4 + 3 * i]) for i in range(nok)]     # (first, count, file)
        at += 1 + 3 * nok
    else:
        res = {"bits": w[0]}
        at = 1
    res["jobs"], at = _checks(w, at)
    assert at == len(w)
    return res


def run(case):
    a, p = _u64(case)
    out = np.zeros(4096, dtype=np.uint64)
    got = load().gzplan_run(p, a.size, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size)
    assert got >= 0, "malformed case"
    return parse(case, out[:got].tolist())


def sanitizer_program(directory):
    """The stand-alone program (-DGZPLAN_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "gzplan_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DGZPLAN_EMUL_MAIN", "-I", CSRC, SRC, "-o", exe])
    return exe


def run_program(exe, cases, directory):
    """The answers of the program to a list of cases; its standard error must stay empty."""
    src, dst = os.path.join(directory, "cases.bin"), os.path.join(directory, "answers.bin")
    with open(src, "wb") as f:
        for case in cases:
            f.write(np.array([len(case)] + list(case), dtype="<u8").tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    w = np.fromfile(dst, dtype="<u8").tolist()
    out, at = [], 0
    for case in cases:
        n = w[at]
        out.append(parse(case, w[at + 1:at + 1 + n]))
        at += 1 + n
    assert at == len(w)
    return out
