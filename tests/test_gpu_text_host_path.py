"""The host path of the calls on record text, on the GPU: the refusal table of tests/textplan_emul_lib.py through the real
entry points (every case returns before a launch), and a three-sample batch -- an empty sample, one of one record, one whose
budget is below its records, more records than chunks -- through screen, spectrum, depth filter and QC in one process,
against the references those calls' own tests use (screen_ref, spectrum_ref, depth_ref, qc_ref)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import depth_ref as D
import qc_ref as Q
import screen_ref as S
import spectrum_ref as R
import textplan_emul_lib as EM
from varkoder_amd import _capi
from varkoder_amd.engine import _u8, _u32, _u64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from varkoder_amd.engine import ImageEngine
    e = ImageEngine(k=7, mapping="cgr", device=0)
    yield e
    e.close()


# ---- the refusal table through the entry points ---------------------------------------------------------------------------
def call_entry(eng, d, call, a):
    """The entry point `call` with check_case's arguments `a`; d: a device tensor that stands for every device pointer (a
    refused call reads and writes none of them).  The workspace is stated as 0 bytes: its size is checked after the rules, so
    a case that the rules let pass is refused there (VK_EINVAL) and nothing is ever launched on these arguments -- which
    also means that only tests/test_textplan_rules.py tells one VK_EINVAL rule from another; here the statuses, and the
    screen's VK_ENOSPC before and after a VK_EINVAL, come from the entry points themselves."""
    L, ctx, p = eng.L, eng.ctx, eng._ptr(d)
    k, every, min_hits = a.get("k", 21), a.get("every", 1), a.get("min_hits", 1)
    if call == EM.SCREEN_BUILD:
        table = a.get("table", True)
        w, dis, st = C.c_uint64(), C.c_uint64(), C.c_uint32()
        return L.vk_screen_build_device(ctx, p, a["length"], k, p if table else None, a.get("table_slots", 1024), p, 0,
                                        C.byref(w), C.byref(dis), C.byref(st))
    n = len(a["offsets"])
    u64 = lambda key: np.ascontiguousarray(a[key], dtype=np.uint64)   # noqa: E731
    offs, lens, recs, nsl, oo = u64("offsets"), u64("lengths"), u64("records"), u64("nslots"), u64("out_offsets")
    lo, hi = np.ascontiguousarray(a["lo"], dtype=np.uint32), np.ascontiguousarray(a["hi"], dtype=np.uint32)
    base, cap = np.zeros(n, dtype=np.uint64), a["out_capacity"]
    if call == EM.EMIT:
        steps = a.get("steps", ())
        ns = len(steps)
        sidx = np.array([s[0] for s in steps] + [0], dtype=np.uint32)
        thr = np.array([s[1] for s in steps] + [0], dtype=np.uint64)
        seeds, whole = np.zeros(ns + 1, dtype=np.uint64), np.zeros(ns + 1, dtype=np.uint8)
        out_offs, out_lens, status = np.zeros(ns + 1, dtype=np.uint64), np.zeros(ns + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        return L.vk_ladder_emit_device(ctx, p, _u64(offs), _u64(lens), _u64(recs), n, _u32(sidx), _u64(seeds), _u64(thr), _u8(whole),
                                       ns, p, 4096, _u64(out_offs), _u64(out_lens), _u32(status), p, 0)
    if call == EM.SCREEN:
        return L.vk_screen_device(ctx, p, _u64(offs), _u64(lens), _u64(recs), n, p, a.get("table_slots", 1024), k, min_hits, 0, p,
                                  _u64(oo), cap, p, p, p, p, 0)
    if call == EM.SPECTRUM:
        return L.vk_spectrum_device(ctx, p, _u64(offs), _u64(lens), _u64(recs), n, k, every, p, p, _u64(base), _u64(nsl), p, p, p,
                                    0)
    if call == EM.SPECTRUM_FASTA:
        return L.vk_spectrum_fasta_device(ctx, p, _u64(offs), _u64(lens), n, k, every, p, p, _u64(base), _u64(nsl), p, p, p, 0)
    if call == EM.DEPTH:
        return L.vk_depth_device(ctx, p, _u64(offs), _u64(lens), _u64(recs), n, k, every, p, p, _u64(base), _u64(nsl), p, _u32(lo),
                                 _u32(hi), p, _u64(oo), cap, p, p, p, p, 0)
    assert call == EM.QC
    return L.vk_qc_device(ctx, p, _u64(offs), _u64(lens), _u64(recs), n, p, p, p, 0)


def test_the_refusal_table_through_the_entry_points(eng):
    import torch
    d = torch.zeros(4096, dtype=torch.uint8, device=eng.device)
    cases = [r for r in EM.REFUSALS if r[4]]
    assert len(cases) >= 60 and {r[1] for r in cases} == set(range(7))
    got = {name: call_entry(eng, d, call, a) for name, call, a, _, _ in cases}
    assert got == {name: status for name, _, _, status, _ in cases}
    assert not d.any()   # (nothing was written)


# ---- three samples, one process, four calls --------------------------------------------------------------------------------
K = 21


def _read(rng, i, n):
    seq = "".join(rng.choice("ACGT") for _ in range(n))
    return f"@r{i}\n{seq}\n+\n{'I' * n}\n".encode()


@functools.lru_cache(maxsize=None)
def batch():
    """(samples, record counts, budgets, reference FASTA): an empty sample, one of one record, one of 12 records whose budget
    is 5.  Two chunks of text and 13 records -- 6 by the budgets --, so the records exceed the chunks either way."""
    rng = random.Random(20240917)
    many = [_read(rng, i, 60 + 3 * i) for i in range(12)]
    many[11] = many[5].replace(b"@r5", b"@r11")   # (a read seen twice: its k-mers' depth is 2)
    one = many[3].replace(b"@r3", b"@only")
    samples = (b"", one, b"".join(many))
    assert sum(-(-len(s) // EM.CHUNK) for s in samples) == 2
    fasta = b">ref\n" + many[3].split(b"\n")[1] + b"\nNN" + many[7].split(b"\n")[1] + b"\n"
    return samples, (0, 1, 12), (0, 1, 5), fasta


@functools.lru_cache(maxsize=None)
def want():
    """The rules' answers: computed once, left unchanged."""
    samples, _, budgets, fasta = batch()
    keys = S.set_ints(fasta, K)
    return {
        "screen": {keep: [S.screen(t, keys, K, 1, keep) for t in samples] for keep in (False, True)},
        "spectrum": [R.spectrum_numpy(t, K) for t in samples],
        "depth": [D.depth_count(t, K, 1, 1, 1) for t in samples],
        "qc_all": Q.rows([(t, Q.record_count(t)) for t in samples]),
        "qc_budget": Q.rows(list(zip(samples, budgets))),
    }


def texts_of(out, offs, lens):
    host = out.cpu().numpy()
    for o, n in zip(offs, lens):   # (zeros up to the 16-byte rounded end)
        assert int(o) % 16 == 0 and not host[int(o) + int(n):(int(o) + int(n) + 15) // 16 * 16].any()
    return [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


def test_three_samples_through_screen_spectrum_depth_and_qc(eng):
    samples, counts, budgets, fasta = batch()
    w = want()
    assert [x[1][0] for x in w["screen"][False]] == list(counts) and w["screen"][True][1][1][1] == 1   # (the one record is in the set)
    dev, offs, lens = eng.upload(list(samples))
    fdev, _, _ = eng.upload([fasta])
    sset = eng.screen_set(fdev, len(fasta), K)
    assert (sset.distinct, sset.windows) == (len(S.set_ints(fasta, K)), S.windows_ints(fasta, K))
    bad = _capi.VK_EM_BAD_RECORDS
    for records, status in ((None, [0, 0, 0]), (list(counts), [0, 0, 0]), (list(budgets), [0, 0, bad])):
        ok = [st == 0 for st in status]
        # screen, both ways
        for keep in (False, True):
            out, ooffs, olens, stats, st = eng.screen(dev, offs, lens, sset, keep=keep, records=records)
            ref = w["screen"][keep]
            assert st.tolist() == status
            assert texts_of(out, ooffs, olens) == [r[0] if f else b"" for r, f in zip(ref, ok)]
            assert stats.tolist() == [r[1] if f else [0, 0, 0, 0] for r, f in zip(ref, ok)]
        # the spectrum, and the depth filter against its tables (band 1..1: the reads whose median k-mer is seen once, so not the read that comes twice)
        rows, st, out, ooffs, olens, drows, bands = eng.spectrum(dev, offs, lens, k=K, records=records, depth=(1, 1))
        assert st.tolist() == status and [b[:3] for b in bands] == [(1, 1, True)] * 3
        zero = [0] * _capi.VK_SPEC_NSTAT
        assert rows.tolist() == [r[0].tolist() if f else zero for r, f in zip(w["spectrum"], ok)]
        assert texts_of(out, ooffs, olens) == [r[0] if f else b"" for r, f in zip(w["depth"], ok)]
        assert drows.tolist() == [r[1].tolist() if f else [0] * _capi.VK_DEPTH_NSTAT for r, f in zip(w["depth"], ok)]
    # QC honours a budget: the first records of a stream
    for records, key in ((None, "qc_all"), (list(counts), "qc_all"), (list(budgets), "qc_budget")):
        rows, st = eng.qc(dev, offs, lens, records=records)
        assert st.tolist() == w[key][1].tolist() == [0, 0, 0]
        assert np.array_equal(rows, w[key][0])
    assert int(w["qc_budget"][0][2][0]) == 5 and int(w["qc_all"][0][2][0]) == 12   # (records counted)
