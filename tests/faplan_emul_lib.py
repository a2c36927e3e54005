"""The host build of the FASTA calls' host rules (tests/emul/faplan_emul.cpp around csrc/vk_faplan.h) as a library that the
tests share: built on first use into tests/emul/ (again when a source is newer), loaded with ctypes.  The sanitizer build is
a program of its own (sanitizer_program) and is never loaded into python.  A case is a flat list of u64 words (clamp_case,
plan_case, pairs_case, first_case, check_case, layout_case); run() answers through the library, run_program() through a
program.  The *_ref functions restate the rules from the comment at the head of csrc/vk_fasta.h and from include/vkimg.h,
not from the header under test; REFUSALS is the table of what the six entry points refuse."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "varkoder_amd", "csrc")
SRC = os.path.join(HERE, "emul", "faplan_emul.cpp")
INCLUDES = ["-I", os.path.join(HERE, "emul", "stub"), "-I", os.path.join(ROOT, "include"), "-I", CSRC]
DEPS = [SRC, os.path.join(ROOT, "include", "vkimg.h")] + [os.path.join(CSRC, h) for h in (
    "vk_faplan.h", "vk_lane.h", "vk_fasta.h", "vk_fasta_ladder.h", "vk_fasta_records.h", "vk_fasta_windows.h", "vk_ws.h")]
VK_OK, VK_EINVAL = 0, 1
LANE, THREADS, SPAN, MAX_STEPS, SUM_CODES = 64, 256, 32, 64, 1024   # kFaLaneBytes, kFaThreads, kFaSpanUnits, kFaMaxSteps, kFawSumCodes
UNIT = LANE * THREADS
NO_SLOT = 0xFFFFFFFF
ENTRY_POINTS = ("vk_count_fasta_device", "vk_count_fasta_sampled_device", "vk_fasta_records_count_device",
                "vk_fasta_records_device", "vk_count_fasta_records_device", "vk_count_fasta_windows_device")
COUNT, SAMPLED, RECORDS_COUNT, RECORDS, COUNT_RECORDS, COUNT_WINDOWS = range(6)
# how far a call came (a check case's answer): refused by its own rules, by the offsets or the sum's grid behind d_fasta,
# by the plan or the pair plan, accepted
RULES_STAGE, OFFSETS_STAGE, PLAN_STAGE, ACCEPTED = range(4)
# the layouts (layout_ref states their pieces)
L_COUNT, L_SAMPLED, L_RECORDS, L_WINDOWS, L_STATE = range(5)

_lib = None


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in DEPS)


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "emul", "libfaplan_emul.so")
    if _stale(so):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + INCLUDES + [SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    u64p = C.POINTER(C.c_uint64)
    L.faplan_run.restype = C.c_int64
    L.faplan_run.argtypes = [u64p, C.c_uint64, u64p, C.c_uint64]
    _lib = L
    return L


# ---- the cases -----------------------------------------------------------------------------------------------------------
def clamp_case(env):
    return [1, int(env)]


def plan_case(override, offsets, lengths):
    assert len(offsets) == len(lengths)
    return [2, int(override), len(offsets)] + [int(x) for x in list(offsets) + list(lengths)]


def pairs_case(override, offsets, lengths, pairs):
    """pairs: (sample, seed, threshold, shift) each."""
    w = plan_case(override, offsets, lengths)
    w[0] = 3
    return w + [len(pairs)] + [int(p[j]) for j in range(4) for p in pairs]


def first_case(rec_first):
    return [4, len(rec_first) - 1] + [int(x) for x in rec_first]


def check_case(call, override=0, offsets=(), lengths=None, rec_first=None, k=7, nslots=2, pairs=(), frag_len=100, win_len=200,
               win_step=100, nrows=4, tile_rows=4, text="ok"):
    """The words of an entry point's argument rules: call one of COUNT .. COUNT_WINDOWS.  What a call does not take stays at
    a value that breaks no rule.  (text: what the entry point is given as d_fasta; the header never sees it.)"""
    n = len(offsets)
    lengths = [0] * n if lengths is None else list(lengths)
    rec_first = list(range(n + 1)) if rec_first is None else list(rec_first)
    assert len(lengths) == n and len(rec_first) == n + 1
    w = [5, call, override, n, int(k) & (2 ** 64 - 1)] + list(offsets) + lengths + rec_first + [nslots, len(pairs)]
    w += [p[j] for j in range(4) for p in pairs] + [frag_len, win_len, win_step, nrows, tile_rows]
    return [int(x) for x in w]


def layout_case(fn, override, lengths, npairs=0, total=0, steps=1, tile_rows=0, k=7):
    return [6, fn, int(override), len(lengths)] + [int(x) for x in lengths] + [npairs, total, steps, tile_rows, k]


def parse(case, w):
    """The answer to a case as a dict (a clamp: the number)."""
    kind = case[0]
    if kind == 1:
        assert len(w) == 1
        return w[0]
    if kind == 2:
        if w[0]:
            assert len(w) == 1
            return {"status": w[0]}
        assert len(w) == 6 + w[5]
        return {"status": 0, "unit": w[1], "span": w[2], "nwg": w[3], "nunits": w[4], "meta": w[6:]}
    if kind == 3:
        assert len(w) == 3 + w[2] + 7
        return {"status": w[0], "pair_nwg": w[1], "words": w[3:3 + w[2]], "view": w[3 + w[2]:]}
    if kind == 4:
        assert len(w) == 1
        return bool(w[0])
    if kind == 5:
        assert len(w) == 4
        return {"status": w[0], "stage": w[1], "steps": w[2], "sum_wgs": w[3]}
    assert len(w) == 2 + 2 * w[1]
    return {"total": w[0], "pieces": [(w[2 + 2 * i], w[3 + 2 * i]) for i in range(w[1])]}


def run(case):
    a = np.ascontiguousarray(case, dtype=np.uint64)
    out = np.zeros(max(4096, 16 * a.size), dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    got = load().faplan_run(a.ctypes.data_as(u64p), a.size, out.ctypes.data_as(u64p), out.size)
    assert got >= 0, "malformed case"
    return parse(case, out[:got].tolist())


def sanitizer_program(directory):
    """The stand-alone program (-DFAPLAN_EMUL_MAIN) built with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(directory, "faplan_emul_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DFAPLAN_EMUL_MAIN"] + INCLUDES + [SRC, "-o", exe])
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


# ---- the rules restated (csrc/vk_fasta.h: "a lane owns kFaLaneBytes of text, a unit is up to kFaThreads lanes
# (VKIMG_FASTA_UNIT_BYTES shrinks it), a workgroup runs over a span of consecutive units of one sample") ---------------------
def clamp_ref(env):
    """0 stays 0; else whole lanes, one at least, a full unit at most."""
    return 0 if env == 0 else min(max(env // LANE * LANE, LANE), UNIT)


def plan_ref(override, offsets, lengths):
    """offsets | lengths | the first workgroup | the first unit of every sample; with the switch set a workgroup takes one
    unit.  Refused: an offset off 16 bytes, a sample of 2^30 units, 2^31 workgroups."""
    unit, span = (override, 1) if override else (UNIT, SPAN)
    wg, first = [0], [0]
    for ln in lengths:
        units = -(-ln // unit)
        wg.append(wg[-1] + -(-units // span))
        first.append(first[-1] + units)
    if any(o % 16 for o in offsets) or any(b - a >= 2 ** 30 for a, b in zip(first, first[1:])) or wg[-1] >= 2 ** 31:
        return {"status": VK_EINVAL}
    return {"status": VK_OK, "unit": unit, "span": span, "nwg": wg[-1], "nunits": first[-1],
            "meta": list(offsets) + list(lengths) + wg + first}


def pairs_ref(plan, pairs):
    """sample | seed | threshold | shift | the first workgroup of every pair: a pair runs its sample's workgroups; the view's
    arrays lie one behind the other."""
    n = len(plan["meta"]) // 4
    wg = plan["meta"][2 * n:3 * n + 1]
    first = [0]
    for p in pairs:
        first.append(first[-1] + wg[p[0] + 1] - wg[p[0]])
    m = len(pairs)
    return {"status": VK_EINVAL if first[-1] >= 2 ** 31 else VK_OK, "pair_nwg": first[-1],
            "words": [p[j] for j in range(4) for p in pairs] + first, "view": [8 * m * j for j in range(5)] + [m, 77]}


def layout_ref(fn, override, lengths, npairs=0, total=0, steps=1, tile_rows=0, k=7):
    """(total, [(name, offset, bytes)]): the pieces one after another, each at a multiple of 256 bytes.  A workspace of the
    context holds the plan's units, one of the caller a unit per lane of text."""
    n = len(lengths)
    unit = override or UNIT
    units = sum(-(-x // (LANE if fn == L_STATE else unit)) for x in lengths)
    lane_words = units * (unit // LANE) + 1
    state = [("meta", 4 * n + 2, 8), ("ukey", units + 1, 4), ("carry", units + 1, 4)]
    pieces = {
        L_COUNT: state,
        L_STATE: state,
        L_SAMPLED: [state[0], ("pairs", 5 * npairs + 1, 8)] + state[1:] + [("unit_ord", units + 1, 8), ("lane", lane_words, 4)],
        L_RECORDS: [state[0], ("rec_first", n + 1, 8)] + state[1:] + [("uhdr", units + 1, 4), ("status", n, 4), ("nrec", n, 4)],
        L_WINDOWS: [("lane", lane_words, 4), ("unit_ord", units + 1, 8), ("bases", n, 8), ("recs", total + 1, 24), ("used", 1, 4),
                    ("tiles", tile_rows * 4 ** k if steps > 1 else 1, 4)],
    }[fn]
    at, out = 0, []
    for name, count, size in pieces:
        out.append((name, at, count * size))
        at += (count * size + 255) // 256 * 256
    return at, out


# ---- the refusal table: every case named by what it shows, with the status the entry point gives --------------------------
# A row: name, call, rule (one of RULES), args (check_case's), status, stage (how far the call comes: tests/test_faplan_rules.py
# asks the header), gpu (the row may go through the real entry point: it returns before a launch -- an accepted neighbour has
# lengths and counts that no text stands behind), resets (the two per-row counting calls: d_hist is zero on return).
RULES = ("none", "k", "offset", "2^30 units", "2^31 workgroups", "frag_len", "pair sample", "pair threshold", "pair shift",
         "pair_nwg", "rec_first", "nslots", "win_step", "win_len 2^31", "win_len multiple", "win_len short", "steps", "nrows",
         "tile_rows", "sum_wgs", "no sample", "d_fasta")
PAIRS = [(0, 1, 2 ** 31, 0), (1, 2, 2 ** 32, 5)]
BIG = 2 ** 30 - 1   # the most units of a sample


def _good(**k):
    """Two samples, two pairs and windows of two tiles that break no rule of any call; one row of output at k = 5 (4096
    bytes), so that a call which resets its output before it refuses resets what the GPU test gives it."""
    a = dict(offsets=[0, 64], lengths=[40, 50], rec_first=[0, 1, 2], k=5, nslots=1, pairs=PAIRS, frag_len=100, win_len=200,
             win_step=100, nrows=1, tile_rows=1)
    a.update(k)
    return a


def _refusals():
    T = []
    name = dict(zip(range(6), ("count", "sampled", "records count", "records", "count records", "count windows")))
    everyone, with_k, with_first, per_row = range(6), (COUNT, SAMPLED, COUNT_RECORDS, COUNT_WINDOWS), (RECORDS, COUNT_RECORDS, COUNT_WINDOWS), \
        (COUNT_RECORDS, COUNT_WINDOWS)

    def row(call, what, rule, args, status, stage, gpu=None):
        gpu = status != VK_OK if gpu is None else gpu
        T.append(dict(name=f"{name[call]}: {what}", call=call, rule=rule, args=args, status=status, stage=stage, gpu=gpu,
                      resets=call in per_row and gpu and stage >= PLAN_STAGE))

    for c in everyone:
        row(c, "no rule broken", "none", _good(), VK_OK, ACCEPTED)
        # the offsets: the plan's rule, and the two per-row counting calls' own ahead of their reset
        st = OFFSETS_STAGE if c in per_row else PLAN_STAGE
        row(c, "the first text at offset 8", "offset", _good(offsets=[8, 64]), VK_EINVAL, st)
        row(c, "the last text at offset 72", "offset", _good(offsets=[0, 72]), VK_EINVAL, st)
        row(c, "texts at offsets 16 and 80", "offset", _good(offsets=[16, 80]), VK_OK, ACCEPTED)
        # the plan: 2^30 units in a sample, 2^31 workgroups in the batch (full units, 32 to a workgroup: 2^25 a sample)
        row(c, "a sample of 2^30 units", "2^30 units", _good(lengths=[40, 2 ** 30 * UNIT]), VK_EINVAL, PLAN_STAGE)
        row(c, "a sample of 2^30 - 1 units", "2^30 units", _good(lengths=[40, BIG * UNIT]), VK_OK, ACCEPTED)
        many = lambda n: dict(offsets=[0] * n, lengths=[BIG * UNIT] * n, rec_first=list(range(n + 1)))   # noqa: E731
        row(c, "2^31 workgroups", "2^31 workgroups", _good(**many(64)), VK_EINVAL, PLAN_STAGE)
        row(c, "2^31 - 2^25 workgroups", "2^31 workgroups", _good(**many(63)), VK_OK, ACCEPTED)
        # ... and with the switch at 64 bytes, a unit to a workgroup (the header alone: the GPU test's engine has full units)
        small = lambda n: dict(override=64, offsets=[0] * n, lengths=[BIG * 64] * n, rec_first=list(range(n + 1)))   # noqa: E731
        row(c, "three samples of 2^30 - 1 units of 64 bytes", "2^31 workgroups", _good(**small(3)), VK_EINVAL, PLAN_STAGE, gpu=False)
        row(c, "two samples of 2^30 - 1 units of 64 bytes", "2^31 workgroups", _good(**small(2)), VK_OK, ACCEPTED)
        # no sample: VK_OK from every call once its rules hold; four of them have not looked at d_fasta, the two per-row
        # counting calls look at it only when there is a sample -- and reset d_hist all the same
        none = dict(offsets=[], lengths=[], rec_first=[0], pairs=[])
        row(c, "no sample", "no sample", _good(**none), VK_OK, ACCEPTED, gpu=True)
        row(c, "no sample and no text", "no sample", _good(text="null", **none), VK_OK, ACCEPTED, gpu=True)
        row(c, "no text", "d_fasta", _good(text="null"), VK_EINVAL, RULES_STAGE)
        row(c, "a text at an odd address", "d_fasta", _good(text="odd"), VK_EINVAL, RULES_STAGE)
    for c in with_k:
        for k in (4, 10):
            row(c, f"k = {k}", "k", _good(k=k, win_step=100), VK_EINVAL, RULES_STAGE)
            # the rules come before the answer to no sample
            row(c, f"k = {k} and no sample", "k", _good(k=k, offsets=[], lengths=[], rec_first=[0], pairs=[]), VK_EINVAL, RULES_STAGE)
        row(c, "k = 9", "k", _good(k=9), VK_OK, ACCEPTED)
    # the sampled call
    c = SAMPLED
    row(c, "frag_len = k - 1", "frag_len", _good(frag_len=4), VK_EINVAL, RULES_STAGE)
    row(c, "frag_len = k", "frag_len", _good(frag_len=5), VK_OK, ACCEPTED)
    row(c, "frag_len = 2^31", "frag_len", _good(frag_len=2 ** 31), VK_EINVAL, RULES_STAGE)
    row(c, "frag_len = 2^31 - 1", "frag_len", _good(frag_len=2 ** 31 - 1), VK_OK, ACCEPTED)
    row(c, "a pair of sample 2 of 2", "pair sample", _good(pairs=[(0, 1, 5, 0), (2, 1, 5, 0)]), VK_EINVAL, RULES_STAGE)
    row(c, "a pair of sample 1 of 2", "pair sample", _good(pairs=[(0, 1, 5, 0), (1, 1, 5, 0)]), VK_OK, ACCEPTED)
    row(c, "a pair and no sample", "pair sample", _good(offsets=[], lengths=[], rec_first=[0], pairs=[(0, 1, 5, 0)]), VK_EINVAL,
        RULES_STAGE)
    row(c, "a threshold of 2^32 + 1", "pair threshold", _good(pairs=[(0, 1, 2 ** 32 + 1, 0)]), VK_EINVAL, RULES_STAGE)
    row(c, "a threshold of 2^32", "pair threshold", _good(pairs=[(0, 1, 2 ** 32, 0)]), VK_OK, ACCEPTED)
    row(c, "a shift of 2^63", "pair shift", _good(pairs=[(0, 1, 5, 2 ** 63)]), VK_EINVAL, RULES_STAGE)
    row(c, "a shift of 2^63 - 1", "pair shift", _good(pairs=[(0, 1, 5, 2 ** 63 - 1)]), VK_OK, ACCEPTED)
    row(c, "no pair", "none", _good(pairs=[]), VK_OK, ACCEPTED)
    big = dict(lengths=[BIG * UNIT, 50])   # sample 0: 2^25 workgroups
    row(c, "pairs of 2^31 workgroups", "pair_nwg", _good(pairs=[(0, 1, 5, 0)] * 64, **big), VK_EINVAL, PLAN_STAGE)
    row(c, "pairs of 2^31 - 2^25 workgroups", "pair_nwg", _good(pairs=[(0, 1, 5, 0)] * 63, **big), VK_OK, ACCEPTED)
    # rec_first
    for c in with_first:
        row(c, "rec_first begins at 1", "rec_first", _good(rec_first=[1, 1, 2]), VK_EINVAL, RULES_STAGE)
        row(c, "rec_first falls", "rec_first", _good(rec_first=[0, 2, 1]), VK_EINVAL, RULES_STAGE)
        row(c, "rec_first stays", "rec_first", _good(rec_first=[0, 1, 1]), VK_OK, ACCEPTED)
        row(c, "rec_first begins at 1 and no sample", "rec_first", _good(offsets=[], lengths=[], rec_first=[1]), VK_EINVAL, RULES_STAGE)
    # the rows of the per-record count
    c = COUNT_RECORDS
    row(c, "no row", "nslots", _good(nslots=0), VK_EINVAL, RULES_STAGE)
    row(c, "2^32 - 1 rows", "nslots", _good(nslots=NO_SLOT), VK_EINVAL, RULES_STAGE)
    row(c, "2^32 - 2 rows", "nslots", _good(nslots=NO_SLOT - 1), VK_OK, ACCEPTED)
    row(c, "a misaligned text and a sample of 2^30 units", "offset", _good(offsets=[0, 72], lengths=[40, 2 ** 30 * UNIT]), VK_EINVAL,
        OFFSETS_STAGE)
    # the windows
    c = COUNT_WINDOWS
    row(c, "win_step = k - 1", "win_step", _good(win_len=8, win_step=4), VK_EINVAL, RULES_STAGE)
    row(c, "win_step = k", "win_step", _good(win_len=10, win_step=5), VK_OK, ACCEPTED)
    row(c, "win_len = 2^31", "win_len 2^31", _good(win_len=2 ** 31, win_step=2 ** 29), VK_EINVAL, RULES_STAGE)
    row(c, "win_len = 2^31 - 2^29", "win_len 2^31", _good(win_len=3 * 2 ** 29, win_step=2 ** 29), VK_OK, ACCEPTED)
    row(c, "win_len = 2.5 win_step", "win_len multiple", _good(win_len=250), VK_EINVAL, RULES_STAGE)
    row(c, "win_len = 3 win_step", "win_len multiple", _good(win_len=300), VK_OK, ACCEPTED)
    row(c, "win_len = win_step / 2", "win_len short", _good(win_len=50), VK_EINVAL, RULES_STAGE)
    row(c, "win_len = 0", "win_len short", _good(win_len=0), VK_EINVAL, RULES_STAGE)
    row(c, "win_len = win_step", "win_len short", _good(win_len=100), VK_OK, ACCEPTED)
    row(c, f"{MAX_STEPS + 1} tiles to a window", "steps", _good(win_len=5 * (MAX_STEPS + 1), win_step=5), VK_EINVAL, RULES_STAGE)
    row(c, f"{MAX_STEPS} tiles to a window", "steps", _good(win_len=5 * MAX_STEPS, win_step=5), VK_OK, ACCEPTED)
    row(c, "no row", "nrows", _good(nrows=0), VK_EINVAL, RULES_STAGE)
    row(c, "one row", "nrows", _good(nrows=1), VK_OK, ACCEPTED)
    row(c, "no tile row, two tiles to a window", "tile_rows", _good(tile_rows=0), VK_EINVAL, RULES_STAGE)
    row(c, "no tile row, one tile to a window", "tile_rows", _good(tile_rows=0, win_len=100), VK_OK, ACCEPTED)
    row(c, "2^31 workgroups of the sum at k = 5", "sum_wgs", _good(tile_rows=2 ** 31), VK_EINVAL, OFFSETS_STAGE)
    row(c, "2^31 - 1 workgroups of the sum at k = 5", "sum_wgs", _good(tile_rows=2 ** 31 - 1), VK_OK, ACCEPTED)
    row(c, "2^31 workgroups of the sum at k = 9", "sum_wgs", _good(k=9, tile_rows=2 ** 23), VK_EINVAL, OFFSETS_STAGE)
    row(c, "2^31 - 256 workgroups of the sum at k = 9", "sum_wgs", _good(k=9, tile_rows=2 ** 23 - 1), VK_OK, ACCEPTED)
    row(c, "a misaligned text and 2^31 workgroups of the sum", "offset", _good(offsets=[8, 64], tile_rows=2 ** 31), VK_EINVAL,
        OFFSETS_STAGE)
    return T


REFUSALS = _refusals()
