"""`--qc-report` on the GPU (vk_qc_device, ImageEngine.qc) against tests/qc_ref.py: rows and status of every stream of
every case of tests/qc_cases.py, exactly -- case by case with the product's merge interval and with 3 records per
workgroup (VKIMG_QC_MERGE), then the whole list as one batch; a 1 MB read in a stream of its own; the error codes."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import qc_cases as QC
import qc_ref as R
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qc_engines():
    """"small" | "default" -> an ImageEngine whose context was made with VKIMG_QC_MERGE = 3 or without it."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(merge):
        if merge not in cache:
            old = os.environ.pop("VKIMG_QC_MERGE", None)
            try:
                if merge == "small":
                    os.environ["VKIMG_QC_MERGE"] = "3"
                cache[merge] = ImageEngine(k=7, mapping="cgr", device=0)
            finally:
                os.environ.pop("VKIMG_QC_MERGE", None)
                if old is not None:
                    os.environ["VKIMG_QC_MERGE"] = old
        return cache[merge]
    yield get
    for e in cache.values():
        e.close()


@functools.lru_cache(maxsize=None)
def want(name):
    """The rule's (rows, status) of a case: computed once, left unchanged."""
    case = next(c for c in QC.all_cases() if c.name == name)
    rows, status = R.rows(case.streams)
    rows.setflags(write=False)
    status.setflags(write=False)
    return case, rows, status


def on_device(eng, buf):
    import torch
    return torch.from_numpy(np.array(buf)).to(eng.device)


def check(got, rows, status, what):
    assert got[1].tolist() == status.tolist(), what
    for j in range(len(rows)):
        assert np.array_equal(got[0][j], rows[j]), (what, j, np.flatnonzero(got[0][j] != rows[j])[:8])


NAMES = [make.__name__ for make in QC.CASES]


@pytest.mark.parametrize("merge", ("default", "small"))
@pytest.mark.parametrize("name", NAMES)
def test_every_case(qc_engines, name, merge):
    eng = qc_engines(merge)
    case, rows, status = want(name)
    buf, offs, lens, recs = QC.pack(case.streams)
    check(eng.qc(on_device(eng, buf), offs, lens, recs), rows, status, name)


def test_the_whole_list_as_one_batch(qc_engines):
    """streams do not leak into each other: every case's streams side by side, the rows unchanged"""
    eng = qc_engines("default")
    parts = [want(n) for n in NAMES]
    streams = [s for case, _, _ in parts for s in case.streams]
    buf, offs, lens, recs = QC.pack(streams)
    got = eng.qc(on_device(eng, buf), offs, lens, recs)
    check(got, np.concatenate([r for _, r, _ in parts]), np.concatenate([s for _, _, s in parts]), "batch")


def test_records_none_counts_every_record(qc_engines):
    eng = qc_engines("default")
    case, rows, status = want("framing")
    buf, offs, lens, _ = QC.pack(case.streams)
    check(eng.qc(on_device(eng, buf), offs, lens), rows, status, "framing, records=None")


def test_a_one_megabyte_read_in_a_stream_of_its_own(qc_engines):
    eng = qc_engines("default")
    streams = [(QC.sweep_record(1 << 20, b"nanopore"), 1), (QC.sweep_record(150, b"short"), 1)]
    rows, status = R.rows(streams)
    assert int(rows[0][R.BASES]) == 1 << 20 and int(rows[0][R.LEN_AT + 1024]) == 1
    buf, offs, lens, recs = QC.pack(streams)
    check(eng.qc(on_device(eng, buf), offs, lens, recs), rows, status, "1 MB read")


def test_an_unaligned_offset_is_refused(qc_engines):
    eng = qc_engines("default")
    case, _, _ = want("framing")
    buf, offs, lens, recs = QC.pack(case.streams[:2])
    offs[1] += np.uint64(8)
    with pytest.raises(_capi.VkError) as e:
        eng.qc(on_device(eng, buf), offs, lens, recs)
    assert e.value.status == _capi.VK_EINVAL


def test_a_workspace_one_byte_short_is_refused(qc_engines):
    import torch
    eng = qc_engines("default")
    case, rows, status = want("framing")
    buf, offs, lens, recs = QC.pack(case.streams)
    dev = on_device(eng, buf)
    n = len(offs)
    u64p = C.POINTER(C.c_uint64)
    need = C.c_uint64()
    assert eng.L.vk_qc_workspace_size(recs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p), n, C.byref(need)) == _capi.VK_OK
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=eng.device)
    out = torch.full((n, _capi.VK_QC_NSTAT), 7, dtype=torch.int64, device=eng.device)
    st = torch.full((n,), 7, dtype=torch.int32, device=eng.device)

    def call(ws_bytes):
        return eng.L.vk_qc_device(eng.ctx, eng._ptr(dev), offs.ctypes.data_as(u64p), lens.ctypes.data_as(u64p),
                                  recs.ctypes.data_as(u64p), n, eng._ptr(out), eng._ptr(st), eng._ptr(ws), ws_bytes)

    assert call(int(need.value) - 1) == _capi.VK_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((st == 7).all())   # (nothing was written)
    assert call(int(need.value)) == _capi.VK_OK
    torch.cuda.synchronize()
    check((out.cpu().numpy().view(np.uint64), st.cpu().numpy().astype(np.uint32)), rows, status, "exact workspace")
