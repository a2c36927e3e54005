"""Adapters by sequence on the MI355X at the boundaries that tests/adapter_cases.py builds.  Detection
(vk_clean_detect_device) gives the planted table of detect_edges() group for group, for every tail trim, and what
adapter_ref gives wherever the test can afford to ask it (every group but the two large pairs, which the CPU tests tie
to the reference); a second call on the same engine and a call with record budgets give the same.  Trimming
(vk_clean_adapters_device) on trim_sweep() equals adapter_ref.clean_sample_adapters in text, stats, status and adapter
stats, padding zero.  A detected table, N included, cleans the reads it came from.  Refused calls leave their outputs
alone.  Byte work: equality everywhere."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_cases as AC  # noqa: E402
import adapter_ref as A  # noqa: E402
import clean_cases as K  # noqa: E402
from gpu_clean_helpers import clean, same, upload  # noqa: E402

from varkoder_amd import _capi  # noqa: E402
from varkoder_amd.engine import _u8, _u32, _u64  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from varkoder_amd.engine import ImageEngine
    e = ImageEngine(k=7, mapping="cgr", device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def edges(eng):
    """detect_edges() in HBM, once for the module: (batch, text tensor, offsets, lengths)."""
    d = AC.detect_edges()
    return (d,) + upload(eng, d)


def detect(eng, b, dev, offs, lens, T, records=None):
    """The single reads' adapter of every sample (no sample here has pairs: those entries are None)."""
    got = eng.detect_adapters(dev, offs, lens, b["records"] if records is None else records, b["roles"], b["owner"],
                              b["nsamples"], trim_tail=T)
    assert len(got) == b["nsamples"] and all(t[:2] == [None, None] for t in got)
    return [t[2] for t in got]


@functools.lru_cache(maxsize=None)
def reference(T):
    """adapter_ref's answer for every group of detect_edges() but the large ones (None there)."""
    d = AC.detect_edges()
    return [None if j in d["large"] else A.group_adapters([], [], [(b"", s, b"") for s in d["reads"][j]], T=T)[2]
            for j in range(d["nsamples"])]


def check_table(d, got, planted, ref):
    by_sample = {j: name for name, j in d["names"].items()}
    for j in range(d["nsamples"]):
        if planted[j] is not AC.FREE:
            assert got[j] == planted[j], f"{by_sample[j]}: {got[j]!r}, planted {planted[j]!r}"
        if j not in d["large"]:
            assert got[j] == ref[j], f"{by_sample[j]}: {got[j]!r}, the reference gives {ref[j]!r}"
        else:
            assert planted[j] is not AC.FREE


@pytest.mark.parametrize("T", AC.TS)
def test_detection_at_the_edges(eng, edges, T):
    d, dev, offs, lens = edges
    assert len(AC.active_groups(d)) > 32                        # two slices
    got = detect(eng, d, dev, offs, lens, T)
    check_table(d, got, d["planted"][T], reference(T))


def test_tail_0_and_1_are_one_shift(eng, edges):
    d, dev, offs, lens = edges
    assert detect(eng, d, dev, offs, lens, 0) == detect(eng, d, dev, offs, lens, 1)


def small_batch():
    b = K.Batch()
    for i, ad in enumerate((A.TRUSEQ1, A.NEXTERA, None)):
        b.add_sample([], [], A.se_readthrough(8500 + i, 700, 0.3 if ad else 0.0, adapter=ad or A.TRUSEQ1, L=90, insert=(25, 50)))
    return b, [A.TRUSEQ1, A.NEXTERA, None]


def test_a_second_call_starts_from_clean_tables(eng, edges):
    """The histograms, the candidates' counts and the occurrence lists of a call are no part of the next one."""
    d, dev, offs, lens = edges
    first = detect(eng, d, dev, offs, lens, 10)
    check_table(d, first, d["planted"][10], reference(10))
    b, want = small_batch()
    sdev, soffs, slens = upload(eng, b)
    assert detect(eng, b, sdev, soffs, slens, 10) == want
    assert [A.group_adapters(*g[:3], T=10)[2] for g in K.groups(b)] == want
    assert detect(eng, d, dev, offs, lens, 10) == first


def test_budgets_end_the_evaluation_set(eng, edges):
    """The evaluation-set groups again with budgets that end 50 / 49 dimers into the second file, well below 262144
    records: the same two answers; every other group as before."""
    d, dev, offs, lens = edges
    records, reads, planted = AC.budget_records(d)
    assert records != d["records"]
    got = detect(eng, d, dev, offs, lens, 10, records=records)
    check_table(d, got, planted, reference(10))
    at, under = d["names"]["eval_at"], d["names"]["eval_under"]
    assert got[at] == d["U"][:A.MAX_DETECTED] and got[under] is None


# ------------------------------------------------------------------ trimming ---

@pytest.mark.parametrize("merge", [True, False])
def test_trim_sweep(eng, merge):
    b = AC.trim_sweep()
    want = AC.sweep_expected(merge)
    got = clean(eng, b, 0, 0, (True, merge, False), adapters=b["adapters"])
    for L in AC.ASSERTED:
        for j in (L - 1, b["dirty"][L]):
            assert len(b["adapters"][j][2]) == L and want[j][3][0] > 20
            same(got[j:j + 1], want[j:j + 1])
    for j, l1, l2 in b["pairs"]:
        assert want[j][3][0] > 60
        same(got[j:j + 1], want[j:j + 1])
    same(got, want)


# ------------------------------------------------------- detect, then clean ---

def chain_batch():
    """The reads of the non-ACGT group and of the four snap groups, as samples of their own."""
    d = AC.detect_edges()
    b = K.Batch()
    want = []
    for name in ["with_n"] + [f"snap_{n}_{nx}" for n, nx in d["snap"]]:
        j = d["names"][name]
        b.add(AC._text(name.encode(), d["reads"][j]), K.SE, b["nsamples"])
        want.append(d["planted"][10][j])
    return b, want


@pytest.mark.parametrize("F,T", [(0, 0), (3, 10)])
def test_detected_table_cleans_its_reads(eng, F, T):
    b, planted = chain_batch()
    dev, offs, lens = upload(eng, b)
    found = eng.detect_adapters(dev, offs, lens, b["records"], b["roles"], b["owner"], b["nsamples"], trim_tail=10)
    assert [t[2] for t in found] == planted and b"N" in planted[0]
    want = []
    for (r1, r2, se, status), t in zip(K.groups(b), found):
        text, st, ad = A.clean_sample_adapters(r1, r2, se, F=F, T=T, adapter=True, merge=True, dedup=False, adapters=t)
        want.append((text, K.stats_words(st), status, [ad["reads"], ad["bases"]]))
    assert all(w[3][0] == len(g[2]) for w, g in zip(want, K.groups(b)))        # every read is cut
    same(clean(eng, b, F, T, (True, True, False), adapters=found), want)


# ----------------------------------------------------------- argument checks ---

SENTINEL = 0xA5


def adapters_call(eng, b, alen, aseq, null=()):
    """vk_clean_adapters_device through eng.L with ImageEngine.clean's marshalling; `null`: arguments passed as null
    pointers.  Returns (status, the output buffers on the host), every output filled with SENTINEL before the call."""
    import torch
    dev, offs, lens = upload(eng, b)
    n = b["nsamples"]
    offs, lens, recs, roles, samples, nfiles, ws = eng._clean_call(offs, lens, b["records"], b["roles"], b["owner"], n,
                                                                   eng.L.vk_clean_workspace_size)
    cap = np.zeros(n, dtype=np.uint64)
    np.add.at(cap, samples.astype(np.int64), lens)
    rounded = (cap + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    out_offs = np.concatenate([[0], np.cumsum(rounded[:-1])]).astype(np.uint64)
    total = int(rounded.sum()) + 16

    def filled(nbytes):
        return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=eng.device)
    outs = dict(out=filled(total), out_lens=filled(8 * n), stats=filled(8 * n * _capi.VK_CL_NSTAT), status=filled(4 * n),
                ad_stats=filled(16 * n))
    st = eng.L.vk_clean_adapters_device(
        eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), _u64(recs), _u32(roles), _u32(samples), nfiles, n, 0, 0,
        _capi.VK_CL_ADAPTER, eng._ptr(ws), ws.numel(), eng._ptr(outs["out"]), _u64(out_offs), total,
        eng._ptr(outs["out_lens"]), eng._ptr(outs["stats"]), eng._ptr(outs["status"]),
        None if "lengths" in null else _u32(alen), None if "seqs" in null else _u8(aseq),
        None if "stats" in null else eng._ptr(outs["ad_stats"]))
    torch.cuda.synchronize()
    return st, {k: v.cpu().numpy() for k, v in outs.items()}


def test_adapters_device_refuses_bad_arguments(eng):
    b, _ = small_batch()
    n = b["nsamples"]
    alen = np.zeros(3 * n, dtype=np.uint32)
    aseq = np.zeros((3 * n, _capi.VK_CL_MAX_ADAPTER), dtype=np.uint8)
    aseq[:] = np.frombuffer((A.TRUSEQ1 * 2)[:_capi.VK_CL_MAX_ADAPTER], dtype=np.uint8)
    alen[2::3] = len(A.TRUSEQ1)
    cases = [("length 65", dict(), _capi.VK_CL_MAX_ADAPTER + 1), ("null lengths", dict(null=("lengths",)), None),
             ("null sequences", dict(null=("seqs",)), None), ("null stats", dict(null=("stats",)), None)]
    for what, kw, long in cases:
        a = alen.copy()
        if long:
            a[3 * n - 1] = long
        st, outs = adapters_call(eng, b, a, aseq, **kw)
        assert st == _capi.VK_EINVAL, what
        for name, buf in outs.items():
            assert (buf == SENTINEL).all(), f"{what}: {name} was written"
    st, outs = adapters_call(eng, b, alen, aseq)        # (the same call with nothing wrong: the marshalling is right)
    assert st == _capi.VK_OK and not (outs["status"] == SENTINEL).all()
    assert outs["ad_stats"].view(np.uint64).reshape(n, 2)[:, 0].tolist()[0] > 100


def test_detect_device_refuses_bad_arguments(eng):
    b, want = small_batch()
    dev, offs, lens = upload(eng, b)
    n = b["nsamples"]
    offs, lens, recs, roles, samples, nfiles, ws = eng._clean_call(offs, lens, b["records"], b["roles"], b["owner"], n,
                                                                   eng.L.vk_clean_detect_workspace_size)
    need = C.c_uint64()
    assert eng.L.vk_clean_detect_workspace_size(_u64(lens), _u64(recs), nfiles, n, C.byref(need)) == _capi.VK_OK
    assert 0 < need.value <= ws.numel()

    def call(null=(), ws_bytes=None):
        alen = np.full(3 * n, 0xA5A5A5A5, dtype=np.uint32)
        aseq = np.full((3 * n, _capi.VK_CL_MAX_ADAPTER), SENTINEL, dtype=np.uint8)
        st = eng.L.vk_clean_detect_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), _u64(recs), _u32(roles),
                                          _u32(samples), nfiles, n, 10, eng._ptr(ws),
                                          need.value if ws_bytes is None else ws_bytes,
                                          None if "lengths" in null else _u32(alen), None if "seqs" in null else _u8(aseq))
        return st, alen, aseq

    for kw in (dict(null=("lengths",)), dict(null=("seqs",)), dict(ws_bytes=need.value - 1), dict(ws_bytes=0)):
        st, alen, aseq = call(**kw)
        assert st == _capi.VK_EINVAL, kw
        assert (alen == 0xA5A5A5A5).all() and (aseq == SENTINEL).all(), kw
    st, alen, aseq = call()
    assert st == _capi.VK_OK
    assert [aseq[3 * j + 2, :alen[3 * j + 2]].tobytes() or None for j in range(n)] == want
