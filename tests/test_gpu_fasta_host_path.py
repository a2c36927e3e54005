"""The host path of the FASTA calls, on the GPU: the refusal table of tests/faplan_emul_lib.py through the six real entry
points (every case returns before a launch; the two per-row counting calls' reset of d_hist ahead of the plan's refusals is
pinned), and one tiny batch -- an empty assembly, one record of 63 bases, five records of 777 bases with an N run and a
lower-case stretch, two records whose second header falls on a 256-byte unit seam -- through all six calls in one process,
with units of 256 bytes and with full units, against the references those calls' own tests use (fasta_ref, fasta_ladder_ref,
fasta_records_ref, fasta_windows_ref)."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import faplan_emul_lib as EM
import fasta_ladder_ref as LR
import fasta_records_ref as RR
import fasta_ref as FR
import fasta_windows_ref as WR
from varkoder_amd.engine import _u32, _u64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa_engines():
    """(k, unit) -> an ImageEngine whose context was made with VKIMG_FASTA_UNIT_BYTES = unit (None: not set)."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(k, unit):
        if (k, unit) not in cache:
            old = os.environ.pop("VKIMG_FASTA_UNIT_BYTES", None)
            if unit is not None:
                os.environ["VKIMG_FASTA_UNIT_BYTES"] = str(unit)
            try:
                cache[(k, unit)] = ImageEngine(k=k, mapping="cgr", device=0)
            finally:
                os.environ.pop("VKIMG_FASTA_UNIT_BYTES", None)
                if old is not None:
                    os.environ["VKIMG_FASTA_UNIT_BYTES"] = old
        return cache[(k, unit)]
    yield get
    for e in cache.values():
        e.close()


# ---- the refusal table through the entry points ---------------------------------------------------------------------------
def call_entry(eng, d, hist, r):
    """The entry point of row r with check_case's arguments; d: a device tensor that stands for every device pointer but
    d_hist (a refused call reads and writes none of them), hist: what the call is given as d_hist.  The host arrays carry
    one entry more than the call is told of, so that none of them is empty."""
    L, ctx, a = eng.L, eng.ctx, r["args"]
    p, h = eng._ptr(d), eng._ptr(hist)
    text = {"ok": p, "null": None, "odd": C.c_void_p(d.data_ptr() + 8)}[a.get("text", "ok")]
    u64 = lambda v: _u64(np.ascontiguousarray(list(v) + [0], dtype=np.uint64))   # noqa: E731
    n, k = len(a["offsets"]), a["k"]
    offs, lens, first = u64(a["offsets"]), u64(a["lengths"]), u64(a["rec_first"])
    call = r["call"]
    if call == EM.COUNT:
        return L.vk_count_fasta_device(ctx, text, offs, lens, n, k, h, p, p)
    if call == EM.SAMPLED:
        pairs = a["pairs"]
        ps = _u32(np.ascontiguousarray([q[0] for q in pairs] + [0], dtype=np.uint32))
        sd, th, sh = (u64([q[j] for q in pairs]) for j in (1, 2, 3))
        return L.vk_count_fasta_sampled_device(ctx, text, offs, lens, n, k, a["frag_len"], len(pairs), ps, sd, th, sh, h, p, p, p)
    if call == EM.RECORDS_COUNT:
        return L.vk_fasta_records_count_device(ctx, text, offs, lens, n, p, p)
    if call == EM.RECORDS:
        return L.vk_fasta_records_device(ctx, text, offs, lens, n, first, p, p, p)
    if call == EM.COUNT_RECORDS:
        return L.vk_count_fasta_records_device(ctx, text, offs, lens, n, k, first, p, a["nslots"], h)
    assert call == EM.COUNT_WINDOWS
    return L.vk_count_fasta_windows_device(ctx, text, offs, lens, n, k, first, p, p, a["win_len"], a["win_step"], 0, a["nrows"],
                                           a["tile_rows"], h)


def test_the_refusal_table_through_the_entry_points(fa_engines):
    import torch
    eng = fa_engines(5, None)   # (full units: the table's plan rows are stated for them)
    d = torch.zeros(4096, dtype=torch.uint8, device=eng.device)
    cases = [r for r in EM.REFUSALS if r["gpu"]]
    assert len(cases) >= 90 and {r["call"] for r in cases} == set(range(6)) and all(r["args"].get("override", 0) == 0 for r in cases)
    got, reset = {}, {}
    for r in cases:
        if r["resets"]:   # one real row at k = 5, 4096 bytes of ones: zero on return, though the call refuses
            assert (r["args"]["k"], r["args"]["nslots"], r["args"]["nrows"]) == (5, 1, 1)
            hist = torch.ones(1024, dtype=torch.int32, device=eng.device)
            got[r["name"]] = call_entry(eng, d, hist, r)
            torch.cuda.synchronize()
            reset[r["name"]] = not bool(hist.any())
        else:
            got[r["name"]] = call_entry(eng, d, d, r)
    torch.cuda.synchronize()
    assert got == {r["name"]: r["status"] for r in cases}
    assert all(reset.values()) and len(reset) >= 8, reset
    assert not d.any()   # (nothing else was written)


# ---- one tiny batch, one process, six calls --------------------------------------------------------------------------------
K, WIN_LEN, WIN_STEP, FRAG = 7, 100, 50, 64
UNITS = (256, None)


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _lines(seq, width=70):
    return "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))


@functools.lru_cache(maxsize=None)
def batch():
    rng = random.Random(20241021)
    one = (">one\n" + _seq(rng, 63) + "\n").encode()
    five = []
    for i in range(5):
        s = _seq(rng, 777)
        if i == 1:
            s = s[:300] + "N" * 40 + s[340:]
        if i == 3:
            s = s[:500] + s[500:650].lower() + s[650:]
        five.append(f">rec{i} of five\n" + _lines(s))
    first = ">a\n" + _lines(_seq(rng, 249))   # 3 + 249 + 4 line ends = 256 bytes: the next header starts a unit of 256
    seam = (first + ">b at the seam\n" + _lines(_seq(rng, 230))).encode()
    assert len(first) == 256 and seam[256:257] == b">"
    return (b"", one, "".join(five).encode(), seam)


# a pair per step of a ladder: every fragment, about half, none; a sample named three times, the empty one once
PAIRS = [(2, 5, LR.ALL, 0), (2, 6, 1 << 31, 9), (1, 5, LR.ALL, 63), (3, 9, 3 << 30, 17), (0, 1, LR.ALL, 0), (2, 7, 0, 0),
         (3, 5, LR.ALL, (1 << 40) + 3)]


@functools.lru_cache(maxsize=None)
def want():
    """The rules' answers: computed once, left unchanged."""
    samples = batch()
    assert [len(RR.table(s)) for s in samples] == [0, 1, 5, 2] and [FR.status(s) for s in samples] == [0, 0, 0, 0]
    return {
        "count": {k: [FR.count(s, k) for s in samples] for k in (K, 9)},
        "sampled": [LR.count(samples[p[0]], K, FRAG, p[1], p[2], p[3]) for p in PAIRS],
        "table": [RR.table(s) for s in samples],
        "records": [RR.count(r, K) for s in samples for r in RR.joined(s)],
        "windows": [WR.rows(s, K, WIN_LEN, WIN_STEP) for s in samples],
    }


@pytest.mark.parametrize("unit", UNITS, ids=["units of 256 bytes", "full units"])
def test_a_tiny_batch_through_the_six_calls(fa_engines, unit):
    import torch
    from varkoder_amd import fasta as VF
    samples, w = batch(), want()
    eng = fa_engines(K, unit)
    buf = eng.upload(list(samples))
    # the plain count, k = 7 and 9
    for k in (K, 9):
        hist, status, bases = fa_engines(k, unit).count_fasta(*buf)
        assert status.tolist() == [0, 0, 0, 0] and bases.tolist() == [c[2] for c in w["count"][k]]
        assert np.array_equal(hist.cpu().numpy().view(np.uint32), np.stack([c[0] for c in w["count"][k]]))
    # the ladder's pairs
    hist, status, bases, taken = eng.count_fasta_sampled(*buf, FRAG, *zip(*PAIRS))
    assert status.tolist() == [0, 0, 0, 0] and bases.tolist() == [FR.bases(s) for s in samples]
    assert taken.tolist() == [p[1] for p in w["sampled"]]
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), np.stack([p[0] for p in w["sampled"]]))
    assert w["sampled"][0][1] == FR.bases(samples[2]) and 0 < w["sampled"][1][1] < FR.bases(samples[2]) and w["sampled"][5][1] == 0
    # the record table (both record calls)
    rec_first, start, rbases, names, status = eng.fasta_records(*buf)
    assert rec_first.tolist() == [0, 0, 1, 6, 8] and status.tolist() == [0, 0, 0, 0]
    got = [(int(start[g]), int(rbases[g]), names[g].ljust(RR.NAME_BYTES, b"\0")) for g in range(8)]
    assert got == [row for t in w["table"] for row in t]
    # a row per record, but one; a spare row stays zero
    slot = np.arange(8, dtype=np.uint32)
    slot[4], slot[5:] = RR.NO_SLOT, slot[5:] - 1
    hist = eng.count_fasta_records(*buf, rec_first, slot, 8).cpu().numpy().view(np.uint32)
    assert np.array_equal(hist[:7], np.stack([r for g, r in enumerate(w["records"]) if g != 4])) and not hist[7].any()
    # the windows, two tiles each: every row, then a range that begins and ends inside records
    counts = VF.window_counts(rbases, WIN_LEN, WIN_STEP)
    assert counts.tolist() == [0] + [14] * 5 + [3, 3] == [r.shape[0] for t in w["windows"] for r in t]
    win_first, _ = VF.window_plan([int(b) for b in rbases], WIN_LEN, WIN_STEP, ncode=4 ** K)
    rows = np.concatenate([r for t in w["windows"] for r in t if r.shape[0]])
    total, m = rows.shape[0], WIN_LEN // WIN_STEP
    hist = eng.count_fasta_windows(*buf, rec_first, rbases, win_first, WIN_LEN, WIN_STEP, 0, total + 1, total + 7 * (m - 1))
    hist = hist.cpu().numpy().view(np.uint32)
    assert np.array_equal(hist[:total], rows) and not hist[total].any()
    part = eng.count_fasta_windows(*buf, rec_first, rbases, win_first, WIN_LEN, WIN_STEP, 10, 25, 25 + 3 * (m - 1))
    assert np.array_equal(part.cpu().numpy().view(np.uint32), rows[10:35])
    torch.cuda.synchronize()
