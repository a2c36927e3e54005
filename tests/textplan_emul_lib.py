"""The host build of the record-text calls' host rules (tests/emul/textplan_emul.cpp around csrc/vk_textplan.h) as a library
that the tests share: built on first use into tests/emul/ (again when a source is newer), loaded with ctypes.  The
sanitizer build is a program of its own (sanitizer_program) and is never loaded into python.  A case is a flat list of u64
words (size_case, index_case, check_case); run() answers through the library, run_program() through a program."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "textplan_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", os.path.join(ROOT, "include"), "-I", CSRC]
DEPS = [SRC, os.path.join(ROOT, "include", "vkimg.h")] + [os.path.join(CSRC, h) for h in (
    "vk_textplan.h", "vk_faplan.h", "vk_clean.h", "vk_emit.h", "vk_lane.h", "vk_fasta.h", "vk_fasta_ladder.h", "vk_fasta_records.h",
    "vk_fasta_windows.h", "vk_screen.h", "vk_spectrum.h", "vk_ws.h")]
CHUNK, SCAN_BLOCK = 16384, 4096   # kClChunk, kClScanBlock
VK_OK, VK_EINVAL, VK_ENOSPC = 0, 1, 6
# the size functions, and the entry points that answer to the same number in a check case
SIZE_FNS = ("vk_ladder_emit_workspace_size", "vk_screen_build_workspace_size", "vk_screen_workspace_size",
            "vk_spectrum_workspace_size", "vk_spectrum_fasta_workspace_size", "vk_depth_workspace_size", "vk_qc_workspace_size")
EMIT, SCREEN_BUILD, SCREEN, SPECTRUM, SPECTRUM_FASTA, DEPTH, QC = range(7)
# the pieces in the order the layouts state them
INDEX_PIECES = ("files", "fchunk", "ccount", "cprefix", "sums", "recs")
FASTA_PIECES = ("meta", "ukey", "carry")
TABLE_PIECES = ("block_base", "slot_base", "nslots")
SCREEN_PIECES = INDEX_PIECES + ("samples", "rec_base", "out_offs", "obytes", "oprefix")
PIECES = {
    EMIT: INDEX_PIECES + ("samples", "status", "steps", "step_base", "sizes", "obytes", "oprefix"),
    SCREEN_BUILD: FASTA_PIECES + ("out", "status"),
    SCREEN: SCREEN_PIECES,
    SPECTRUM: INDEX_PIECES + ("samples", "rec_base") + TABLE_PIECES,
    SPECTRUM_FASTA: FASTA_PIECES + TABLE_PIECES,
    DEPTH: SCREEN_PIECES + ("slot_base", "nslots", "lo", "hi"),
    QC: INDEX_PIECES + ("streams", "block_base", "bad"),
}

_lib = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "emul", "libtextplan_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCLUDES + [SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    u64p = C.POINTER(C.c_uint64)
    L.textplan_run.restype = C.c_int64
    L.textplan_run.argtypes = [u64p, C.c_uint64, u64p, C.c_uint64]
    _lib = L
    return L


def size_case(fn, lengths=(), records=(), step_sample=(), length=0):
    """The words of a *_workspace_size call: fn one of EMIT .. QC, with the arrays that function takes."""
    if fn == SCREEN_BUILD:
        return [1, fn, int(length)]
    w = [1, fn, len(lengths)] + ([len(step_sample)] if fn == EMIT else []) + list(lengths)
    if fn != SPECTRUM_FASTA:
        assert len(records) == len(lengths)
        w += list(records)
    return [int(x) for x in w + (list(step_sample) if fn == EMIT else [])]


def index_case(offsets, lengths, records):
    assert len(offsets) == len(lengths) == len(records)
    return [2, len(offsets)] + [int(x) for x in list(offsets) + list(lengths) + list(records)]


def check_case(call, offsets=(), lengths=None, records=None, nslots=None, out_offsets=None, out_capacity=0, lo=None, hi=None,
               k=21, every=1, min_hits=1, table_slots=1024, per_block=512, steps=(), length=0, table=True):
    """The words of an entry point's argument rules: call one of EMIT .. QC.  What a call does not take stays at a value
    that breaks no rule.  steps: (sample, threshold) of a ladder emit; length, table, table_slots: a screen build's."""
    if call == SCREEN_BUILD:
        return [3, call, int(length), int(k) & (2 ** 64 - 1), int(table), int(table_slots)]
    n = len(offsets)
    fill = lambda v, d: [d] * n if v is None else list(v)   # noqa: E731
    extra = per_block if call == QC else table_slots
    w = [3, call, n, int(k) & (2 ** 64 - 1), every, min_hits, out_capacity, extra]
    w += list(offsets) + fill(lengths, 0) + fill(records, 0) + fill(nslots, 1024) + fill(out_offsets, 0) + fill(lo, 0) + fill(hi, 0)
    if call == EMIT:
        w += [len(steps)] + [s[0] for s in steps] + [s[1] for s in steps]
    return [int(x) for x in w]


def parse(case, w):
    """The answer to a case as a dict."""
    kind = case[0]
    if kind == 1:
        names = PIECES[case[1]]
        assert w[1] == len(names) and len(w) == 2 + 2 * len(names)
        return {"total": w[0], "pieces": [(name, w[2 + 2 * i], w[3 + 2 * i]) for i, name in enumerate(names)]}
    if kind == 2:
        n = case[1]
        assert len(w) == 2 + 6 * n + n + 1 + 5 * n + n
        rows = [dict(zip(("off", "len", "rec0", "nrec", "chunk0", "chunk1"), w[2 + 6 * i:8 + 6 * i])) for i in range(n)]
        at = 2 + 6 * n
        files = [dict(zip(("off", "len", "nrec", "rec0", "chunk0"), w[at + n + 1 + 5 * i:at + n + 6 + 5 * i])) for i in range(n)]
        return {"nchunks": w[0], "nrec": w[1], "rows": rows, "rec_base": w[at:at + n + 1], "files": files, "fchunk": w[at + 6 * n + 1:]}
    assert len(w) == 2 + w[1]
    return {"status": w[0], "block_base": w[2:]}


def run(case):
    a = np.ascontiguousarray(case, dtype=np.uint64)
    out = np.zeros(max(4096, 16 * a.size), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    got = load().textplan_run(a.ctypes.data_as(u64p), a.size, out.ctypes.data_as(u64p), out.size)
    assert got >= 0, "malformed case"
    return parse(case, out[:got].tolist())


def sanitizer_program(directory):
    """The stand-alone program (-DTEXTPLAN_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "textplan_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DTEXTPLAN_EMUL_MAIN"] + INCLUDES + [SRC, "-o", exe])
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


# ---- the refusal table: every case named by the rule it breaks, with the status the entry point gives -------------------
# (name, call, check_case's arguments, status, reaches the GPU test).  tests/test_textplan_rules.py asks the header,
# tests/test_gpu_text_host_path.py the entry points: there only the refused cases go (every one returns before a launch);
# a neighbour that is accepted has lengths and counts that no text stands behind.
def _good(**k):
    """Two samples that break no rule of any call: texts at 0 and 64, regions of 48 and 64 bytes in 112."""
    a = dict(offsets=[0, 64], lengths=[40, 50], records=[1, 1], nslots=[1024, 1024], out_offsets=[0, 48], out_capacity=112,
             lo=[1, 1], hi=[5, 5])
    a.update(k)
    return a


def _refusals():
    T = []
    text_calls = (EMIT, SCREEN, SPECTRUM, SPECTRUM_FASTA, DEPTH, QC)
    name = {EMIT: "emit", SCREEN_BUILD: "screen build", SCREEN: "screen", SPECTRUM: "spectrum", SPECTRUM_FASTA: "spectrum fasta",
            DEPTH: "depth", QC: "qc"}
    for c in text_calls:
        T.append((f"{name[c]}: no rule broken", c, _good(), VK_OK, False))
        T.append((f"{name[c]}: a text at offset 8", c, _good(offsets=[0, 8]), VK_EINVAL, True))
    for c in (SPECTRUM, SPECTRUM_FASTA, DEPTH):
        big = dict(out_offsets=[0, 48], out_capacity=2 ** 34)
        T.append((f"{name[c]}: a sample of 2^33 bytes", c, _good(lengths=[40, 2 ** 33], **big), VK_OK, False))
        T.append((f"{name[c]}: a sample of 2^33 + 1 bytes", c, _good(lengths=[40, 2 ** 33 + 1], **big), VK_EINVAL, True))
    for c in (EMIT, SCREEN):
        T.append((f"{name[c]}: no cap on a sample's bytes", c, _good(lengths=[40, 2 ** 33 + 1], out_capacity=2 ** 34), VK_OK, False))
    T.append(("qc: a stream of 2^32 - 1 bytes", QC, _good(lengths=[40, 2 ** 32 - 1]), VK_OK, False))
    T.append(("qc: a stream of 2^32 bytes", QC, _good(lengths=[40, 2 ** 32]), VK_EINVAL, True))
    for slots in (512, 1025, 2 ** 41):
        for c in (SPECTRUM, SPECTRUM_FASTA, DEPTH):
            T.append((f"{name[c]}: a table of {slots} slots", c, _good(nslots=[1024, slots]), VK_EINVAL, True))
        T.append((f"screen: a table of {slots} slots", SCREEN, _good(table_slots=slots), VK_EINVAL, True))
        T.append((f"screen build: a table of {slots} slots", SCREEN_BUILD, dict(length=100, table_slots=slots), VK_EINVAL, True))
    T.append(("screen build: a table of 2^40 slots", SCREEN_BUILD, dict(length=100, table_slots=2 ** 40), VK_OK, False))
    T.append(("screen build: slots without a table", SCREEN_BUILD, dict(length=100, table=False, table_slots=1024), VK_EINVAL, True))
    T.append(("screen build: a table without slots", SCREEN_BUILD, dict(length=100, table=True, table_slots=0), VK_EINVAL, True))
    T.append(("screen build: the windows only", SCREEN_BUILD, dict(length=100, table=False, table_slots=0), VK_OK, False))
    T.append(("screen build: a reference of 2^30 + 1 bytes", SCREEN_BUILD, dict(length=2 ** 30 + 1), VK_EINVAL, True))
    for k in (15, 32):
        for c in (SCREEN, SPECTRUM, SPECTRUM_FASTA, DEPTH):
            T.append((f"{name[c]}: k = {k}", c, _good(k=k), VK_EINVAL, True))
        T.append((f"screen build: k = {k}", SCREEN_BUILD, dict(length=100, k=k), VK_EINVAL, True))
    for k in (16, 31):
        T.append((f"spectrum: k = {k}", SPECTRUM, _good(k=k), VK_OK, False))
    for c in (SPECTRUM, SPECTRUM_FASTA, DEPTH):
        T.append((f"{name[c]}: every = 0", c, _good(every=0), VK_EINVAL, True))
    T.append(("screen: min_hits = 0", SCREEN, _good(min_hits=0), VK_EINVAL, True))
    T.append(("depth: lo above hi", DEPTH, _good(lo=[1, 6]), VK_EINVAL, True))
    T.append(("depth: lo equal to hi", DEPTH, _good(lo=[1, 5]), VK_OK, False))
    # the known wart: one status from the screen, another from the depth filter
    T.append(("screen: a region one 16-byte step short", SCREEN, _good(out_capacity=96), VK_ENOSPC, True))
    T.append(("depth: a region one 16-byte step short", DEPTH, _good(out_capacity=96), VK_EINVAL, True))
    T.append(("screen: a region past the output", SCREEN, _good(out_offsets=[0, 128]), VK_ENOSPC, True))
    for c in (SCREEN, DEPTH):
        T.append((f"{name[c]}: a region at offset 56", c, _good(out_offsets=[0, 56], out_capacity=128), VK_EINVAL, True))
    # the grids: 2^31 workgroups are refused, one fewer is not
    full = [2 ** 40] * 32   # 2^26 workgroups of 16,384 slots each
    many = dict(offsets=[0] * 32, lengths=[0] * 32, records=[0] * 32, out_offsets=[0] * 32, lo=[1] * 32, hi=[1] * 32)
    for c in (SPECTRUM, SPECTRUM_FASTA):
        T.append((f"{name[c]}: 2^31 workgroups of slots", c, _good(nslots=full, **many), VK_EINVAL, True))
        T.append((f"{name[c]}: 2^31 - 2^25 workgroups of slots", c, _good(nslots=full[:-1] + [2 ** 39], **many), VK_OK, False))
    for c in (SPECTRUM, DEPTH):
        T.append((f"{name[c]}: 2^31 workgroups of records", c, _good(records=[1, 2 ** 37 - 1]), VK_EINVAL, True))
        T.append((f"{name[c]}: 2^31 - 1 workgroups of records", c, _good(records=[1, 2 ** 37 - 65]), VK_OK, False))
    T.append(("screen: no limit on the records' workgroups", SCREEN, _good(records=[1, 2 ** 37 - 1]), VK_OK, False))
    T.append(("qc: 2^31 workgroups of records", QC, _good(records=[512, 2 ** 40 - 512]), VK_EINVAL, True))
    T.append(("qc: 2^31 - 1 workgroups of records", QC, _good(records=[512, 2 ** 40 - 1024]), VK_OK, False))
    # the ladder's steps
    T.append(("emit: steps in range", EMIT, _good(steps=[(0, 2 ** 32), (1, 5)]), VK_OK, False))
    T.append(("emit: a step of sample 2 of 2", EMIT, _good(steps=[(0, 5), (2, 5)]), VK_EINVAL, True))
    T.append(("emit: a threshold of 2^32 + 1", EMIT, _good(steps=[(0, 2 ** 32 + 1)]), VK_EINVAL, True))
    # two rules at once: the first sample that breaks one decides, and within a sample the region comes last
    T.append(("screen: sample 0's region short, sample 1's text at offset 8", SCREEN,
              _good(offsets=[0, 8], out_capacity=32), VK_ENOSPC, True))
    T.append(("screen: sample 0's text at offset 8, sample 1's region short", SCREEN,
              _good(offsets=[8, 64], out_capacity=96), VK_EINVAL, True))
    T.append(("screen: sample 1's region misaligned and short", SCREEN, _good(out_offsets=[0, 56], out_capacity=96), VK_EINVAL, True))
    T.append(("screen: k = 15 and a region short", SCREEN, _good(k=15, out_capacity=96), VK_EINVAL, True))
    T.append(("depth: a region short and lo above hi", DEPTH, _good(out_capacity=96, lo=[6, 1]), VK_EINVAL, True))
    return T


REFUSALS = _refusals()
