"""The host build of the BAM calls' host rules (tests/emul/bamplan_emul.cpp around csrc/vk_bamplan.h) as a library that the
tests share: built on first use into tests/emul/ (again when a source is newer), loaded with ctypes.  The sanitizer build
is a program of its own (sanitizer_program) and is never loaded into python.  A case is a flat list of u64 words
(args_case, plan_case, describe_case, pick_case, status_case, slot_case); run() answers through the library,
run_program() through a program."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "bamplan_emul.cpp")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("vk_bamplan.h", "vk_bam.h", "vk_bam_groups.h", "vk_ws.h")]
ALL, READ1, READ2, SINGLE = 0, 1, 2, 3   # VK_BAM_ALL .. VK_BAM_SINGLE
UNGROUPED = 0xFFFFFFFF                   # VK_BAM_UNGROUPED
NO_STREAM = 0xFFFF                       # kBamNoStream
NO_GUESS = 1                             # VK_BAM_NO_GUESS
# the descriptor block's pieces in the order bg_take states them, with their element sizes
PIECES = (("ids", 1), ("group_first", 4), ("id_first", 4), ("slots", 4), ("slot_first", 4), ("map_first", 4), ("ls_first", 4),
          ("ls_stream", 4), ("stream_file", 4), ("stream_local", 4), ("map", 2), ("pan_first", 8), ("row_first", 8),
          ("out_offs", 8), ("out_caps", 8))

_lib = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "emul", "libbamplan_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    u64p = C.POINTER(C.c_uint64)
    L.bamplan_run.restype = C.c_int64
    L.bamplan_run.argtypes = [u64p, C.c_uint64, u64p, C.c_uint64]
    _lib = L
    return L


def call(lengths, streams=(), groups=None, flags=0, slots=None, group_first=None, id_first=None):
    """The words of a call.  lengths: the files' inflated bytes; streams: (file, select) or, with groups, (file, select,
    group); groups: per file the list of its IDs (bytes), None for an ungrouped call; slots: per stream (offset, cap), None
    for a framing call; group_first, id_first: in place of what `groups` gives (to state a malformed call)."""
    w = [len(lengths), len(streams), flags, int(groups is not None), int(slots is not None)]
    w += list(lengths) + [s[0] for s in streams] + [s[1] for s in streams]
    if groups is not None:
        ids = [bytes(i) for g in groups for i in g]
        gf = list(np.cumsum([0] + [len(g) for g in groups])) if group_first is None else list(group_first)
        idf = list(np.cumsum([0] + [len(i) for i in ids])) if id_first is None else list(id_first)
        raw = b"".join(ids)
        w += [s[2] for s in streams] + gf + [len(idf)] + idf + [len(raw)] + list(raw)
    if slots is not None:
        w += [s[0] for s in slots] + [s[1] for s in slots]
    return [int(x) for x in w]


def args_case(*a, **k):
    return [1] + call(*a, **k)


def plan_case(seg_bytes, *a, **k):
    return [2, seg_bytes] + call(*a, **k)


def describe_case(seg, panel, lengths, streams, groups, queries=(), slots=None):
    """queries: (file, ID bytes) for the product's probe over the file's table."""
    w = [3, seg, panel] + call(lengths, streams, groups, slots=slots) + [len(queries)]
    for f, v in queries:
        w += [f, len(v)] + list(v)
    return w


def pick_case(v, select):
    return [4, 0] + list(v) + [select]


def status_case(status, aux_bad):
    return [4, 1, status, aux_bad]


def slot_case(n, cap):
    return [4, 2, n, cap]


def parse(case, w):
    """The answer to a case as a dict."""
    kind = case[0]
    if kind == 1:
        assert len(w) == 2
        return {"bam_args_ok": bool(w[0]), "bg_args_ok": bool(w[1])}
    if kind == 2:
        nfiles = case[2]
        res = dict(zip(("ok", "seg", "nstreams", "segs", "stream_segs"), w[:5]))
        ns, at = res["nstreams"], 5
        for key, n in (("seg_first", nfiles + 1), ("sseg_first", ns + 1), ("out_offs", ns), ("out_caps", ns)):
            res[key] = w[at:at + n]
            at += n
        assert at == len(w)
        return res
    if kind == 3:
        res = {"workspace": w[0], "desc_bytes": w[1], "back_bytes": w[2], "at": {}}
        at = 3
        for name, _ in PIECES:
            res["at"][name] = w[at]
            res[name] = w[at + 2:at + 2 + w[at + 1]]
            at += 2 + w[at + 1]
        res["found"] = w[at:]
        return res
    if case[1] == 2:
        return {"fits": bool(w[0]), "length": w[1]}
    assert len(w) == 1
    return w[0]


def run(case):
    a = np.ascontiguousarray(case, dtype=np.uint64)
    out = np.zeros(max(4096, 2 * a.size + 65536), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    got = load().bamplan_run(a.ctypes.data_as(u64p), a.size, out.ctypes.data_as(u64p), out.size)
    assert got >= 0, "malformed case"
    return parse(case, out[:got].tolist())


def sanitizer_program(directory):
    """The stand-alone program (-DBAMPLAN_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "bamplan_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DBAMPLAN_EMUL_MAIN", "-I", CSRC, SRC, "-o", exe])
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
