"""`--genome-spectrum` on the GPU: vk_spectrum_fasta_device and ImageEngine.spectrum_fasta against
tests/fasta_spectrum_ref.py -- rows, statuses and the tables' held (key, count) pairs equal -- with VKIMG_FASTA_UNIT_BYTES
small in one engine and at its default in another; a table that fills, the engine's recount, groups, sketches and the
error codes.  Every case of fasta_spectrum_cases.py runs at K = 16, 21, 31 and every = 1, 4."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fasta_spectrum_cases as FC
import fasta_spectrum_ref as FR
import sketch_ref as R

pytestmark = pytest.mark.gpu

UNITS = ("small", "default")
EMPTY = np.uint64(2 ** 64 - 1)


@pytest.fixture(scope="module")
def engines():
    """"small" | "default" -> an ImageEngine whose context was made with VKIMG_FASTA_UNIT_BYTES = 256 or unset."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(unit):
        if unit not in cache:
            old = os.environ.pop("VKIMG_FASTA_UNIT_BYTES", None)
            try:
                if unit == "small":
                    os.environ["VKIMG_FASTA_UNIT_BYTES"] = str(FC.SMALL_UNIT)
                cache[unit] = ImageEngine(k=7, mapping="cgr", device=0)   # (the image's k and mapping are not used)
            finally:
                os.environ.pop("VKIMG_FASTA_UNIT_BYTES", None)
                if old is not None:
                    os.environ["VKIMG_FASTA_UNIT_BYTES"] = old
        return cache[unit]
    yield get
    for e in cache.values():
        e.close()


@functools.lru_cache(maxsize=None)
def expected(k, every):
    """[(name, text, row, status, keys, counts)] by the rule's second statement: computed once, shared, left unchanged."""
    return [(name, text) + FR.spectrum_numpy(text, k, every) for name, text in FC.cases(k)]


def call(eng, samples, k, every, nslots, sketch=None):
    """vk_spectrum_fasta_device on a batch: (rows, status, [sorted held keys and their counts], sketches or None)."""
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import _u64
    dev, offs, lens = eng.upload(samples)
    n = len(samples)
    nsl = np.asarray(nslots, dtype=np.uint64)
    base = np.zeros(n, dtype=np.uint64)
    base[1:] = np.cumsum(nsl[:-1])
    keys = torch.empty(int(nsl.sum()), dtype=torch.int64, device=eng.device)
    counts = torch.empty(int(nsl.sum()), dtype=torch.int32, device=eng.device)
    ws_bytes = C.c_uint64()
    _capi.check(eng.ctx, eng.L.vk_spectrum_fasta_workspace_size(_u64(lens), n, C.byref(ws_bytes)), "workspace")
    ws = torch.empty(max(int(ws_bytes.value), 256), dtype=torch.uint8, device=eng.device)
    d_rows = torch.empty((n, _capi.VK_SPEC_NSTAT), dtype=torch.int64, device=eng.device)
    d_status = torch.empty(n, dtype=torch.int32, device=eng.device)
    st = eng.L.vk_spectrum_fasta_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), n, k, every, eng._ptr(keys),
                                        eng._ptr(counts), _u64(base), _u64(nsl), eng._ptr(d_rows), eng._ptr(d_status),
                                        eng._ptr(ws), ws.numel())
    _capi.check(eng.ctx, st, "vk_spectrum_fasta_device")
    sk = eng.sketch_tables(keys, counts, base, nsl, d_status, sketch, 1) if sketch else None
    hk, hc = keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32)
    tables = []
    for b, m in zip(base, nsl):
        tk, tc = hk[int(b):int(b + m)], hc[int(b):int(b + m)]
        held = tk != EMPTY
        assert not tc[~held].any()   # (a free slot counts nothing)
        order = np.argsort(tk[held])
        tables.append((tk[held][order], tc[held][order]))
    return d_rows.cpu().numpy().view(np.uint64), d_status.cpu().numpy().view(np.uint32), tables, sk


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("every", FC.EVERIES)
@pytest.mark.parametrize("k", FC.KS)
def test_rows_status_and_tables_equal_the_rule(engines, k, every, unit):
    """Every case in one batch: line widths at every phase of a lane, CRLF, no final newline, headers in the middle and on
    the last byte of a lane, '>' alone, two in a row, longer than a unit, at the text's end, N every K - 1 / K / K + 1,
    lower case, IUPAC, records of K - 1 and K bases, a palindrome, a record and its reverse complement, poly-A, tandem
    repeats, the empty text and a bad start -- and the sketch of each from the tables as they lie."""
    want = expected(k, every)
    texts = [t for _, t, *_ in want]
    rows, status, tables, sk = call(engines(unit), texts, k, every, [FR.slots_for(len(t), 1) for t in texts], sketch=64)
    for i, (name, _, wrow, wst, wkeys, wcounts) in enumerate(want):
        assert int(status[i]) == wst, name
        assert np.array_equal(rows[i], wrow), name
        if wst == 0:
            assert np.array_equal(tables[i][0], wkeys) and np.array_equal(tables[i][1], wcounts.astype(np.uint32)), name
            h, eligible = R.sketch_np(wkeys, wcounts, 1, 64)
            assert np.array_equal(sk[0][i], R.row(h, 64)) and sk[1][i].tolist() == [eligible, len(h)], name


@pytest.mark.parametrize("unit", UNITS)
def test_the_engine_on_a_batch_with_a_bad_start_and_an_empty_sample(engines, unit):
    k = 21
    eng = engines(unit)
    batch = FC.batch(k)
    dev, offs, lens = eng.upload([t for _, t in batch])
    rows, status, hashes, info = eng.spectrum_fasta(dev, offs, lens, k=k, sketch=(64, 1))
    for i, (name, text) in enumerate(batch):
        wrow, wst, wkeys, wcounts = FR.spectrum_numpy(text, k)
        assert int(status[i]) == wst and np.array_equal(rows[i], wrow), name
        h, eligible = R.sketch_np(wkeys, wcounts, 1, 64)
        assert np.array_equal(hashes[i], R.row(h, 64)) and info[i].tolist() == [eligible, len(h)], name
    assert status.tolist() == [0, FR.VK_ST_BAD_START, 0, 0, 0] and not rows[1].any() and not rows[3].any()
    # each sample alone gives the same row
    for i in (0, 2, 4):
        r1, s1 = eng.spectrum_fasta(*eng.upload([batch[i][1]]), k=k)
        assert s1.tolist() == [0] and np.array_equal(r1[0], rows[i])
    assert eng.spectrum_fasta(dev, offs[:0], lens[:0])[0].shape == (0, FR.NSTAT)


@functools.lru_cache(maxsize=None)
def random_samples():
    rng = np.random.default_rng(77)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [FC.fa([(b"c%d" % j, letters[rng.integers(0, 4, 25000)].tobytes()) for j in range(2)], 60 + i) for i in range(3)]


@pytest.mark.parametrize("unit", UNITS)
def test_a_full_table_is_a_status_and_its_neighbour_is_unchanged(engines, unit):
    k = 21
    big, small = random_samples()[0], dict(FC.cases(k))["width_61"]
    rows, status, tables, _ = call(engines(unit), [small, big, small], k, 1, [1024, 1024, 2048])
    wrow, _, wkeys, wcounts = FR.spectrum_numpy(small, k)
    assert status.tolist() == [0, FR.VK_SPEC_TABLE_FULL, 0] and not rows[1].any()
    for i in (0, 2):
        assert np.array_equal(rows[i], wrow) and np.array_equal(tables[i][0], wkeys) and np.array_equal(tables[i][1], wcounts)
    assert FR.spectrum_numpy(big, k, 1, slots=1024)[1] == FR.VK_SPEC_TABLE_FULL


def test_a_sample_whose_first_table_fills_is_counted_again(engines):
    """every = 16 on a text built so that more than a fifth of its windows are taken (selection is by key): the first table
    of slots_for(length, 16) fills, the engine counts again with four times the slots."""
    k, every = 21, 16
    text = FC.dense_taken(k, every, 65000)
    wrow, wst, wkeys, wcounts = FR.spectrum_numpy(text, k, every)
    first = FR.slots_for(len(text), every)
    assert wst == 0 and len(wkeys) > first   # (the first table must fill)
    eng = engines("default")
    dev, offs, lens = eng.upload([text])
    rows, status, hashes, info = eng.spectrum_fasta(dev, offs, lens, k=k, every=every, sketch=(64, 1))
    assert status.tolist() == [0] and np.array_equal(rows[0], wrow)
    h, eligible = R.sketch_np(wkeys, wcounts, 1, 64)
    assert np.array_equal(hashes[0], R.row(h, 64)) and info[0].tolist() == [eligible, len(h)]
    # forced to the first size it stays full
    _, st = eng.spectrum_fasta(dev, offs, lens, k=k, every=every, slots=first)
    assert st.tolist() == [FR.VK_SPEC_TABLE_FULL]


def test_one_group_and_two_give_equal_results(engines):
    k = 21
    eng = engines("default")
    samples = random_samples()
    dev, offs, lens = eng.upload(samples)
    one = eng.spectrum_fasta(dev, offs, lens, k=k, sketch=(1024, 1))
    slots = FR.slots_for(len(samples[0]))
    two = eng.spectrum_fasta(dev, offs, lens, k=k, sketch=(1024, 1), table_bytes=2 * slots * 12)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    for i, text in enumerate(samples):
        wrow, wst, wkeys, wcounts = FR.spectrum_numpy(text, k)
        assert one[1][i] == 0 and np.array_equal(one[0][i], wrow)
        h, eligible = R.sketch_np(wkeys, wcounts, 1, 1024)
        assert np.array_equal(one[2][i], R.row(h, 1024)) and one[3][i].tolist() == [eligible, len(h)]


def test_error_codes(engines):
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import _u64
    eng = engines("default")
    text = dict(FC.cases(21))["width_60"]
    dev, offs, lens = eng.upload([text, text])
    n = 2
    nsl = np.array([1024, 1024], dtype=np.uint64)
    base = np.array([0, 1024], dtype=np.uint64)
    keys = torch.empty(2048, dtype=torch.int64, device=eng.device)
    counts = torch.empty(2048, dtype=torch.int32, device=eng.device)
    ws_bytes = C.c_uint64()
    assert eng.L.vk_spectrum_fasta_workspace_size(_u64(lens), n, C.byref(ws_bytes)) == 0
    assert eng.L.vk_spectrum_fasta_workspace_size(_u64(lens), n, None) == _capi.VK_EINVAL
    assert eng.L.vk_spectrum_fasta_workspace_size(None, n, C.byref(ws_bytes)) == _capi.VK_EINVAL
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=eng.device)
    rows = torch.zeros((n, _capi.VK_SPEC_NSTAT), dtype=torch.int64, device=eng.device)
    status = torch.zeros(n, dtype=torch.int32, device=eng.device)

    def run(**ch):
        a = dict(ctx=eng.ctx, text=eng._ptr(dev), offs=_u64(offs), lens=_u64(lens), n=n, k=21, every=1, keys=eng._ptr(keys),
                 counts=eng._ptr(counts), base=_u64(base), nsl=_u64(nsl), rows=eng._ptr(rows), status=eng._ptr(status),
                 ws=eng._ptr(ws), ws_bytes=ws.numel())
        a.update(ch)
        return eng.L.vk_spectrum_fasta_device(a["ctx"], a["text"], a["offs"], a["lens"], a["n"], a["k"], a["every"], a["keys"],
                                              a["counts"], a["base"], a["nsl"], a["rows"], a["status"], a["ws"], a["ws_bytes"])
    assert run() == 0
    for name in ("ctx", "text", "offs", "lens", "keys", "counts", "base", "nsl", "rows", "status", "ws"):
        assert run(**{name: None}) == _capi.VK_EINVAL, name
    assert run(n=0) == _capi.VK_EINVAL
    assert run(k=15) == _capi.VK_EINVAL and run(k=32) == _capi.VK_EINVAL
    assert run(every=0) == _capi.VK_EINVAL
    assert run(nsl=_u64(np.array([1024, 512], dtype=np.uint64))) == _capi.VK_EINVAL
    assert run(nsl=_u64(np.array([1024, 1025], dtype=np.uint64))) == _capi.VK_EINVAL
    assert run(offs=_u64(np.array([0, int(offs[1]) + 8], dtype=np.uint64))) == _capi.VK_EINVAL
    assert run(lens=_u64(np.array([int(lens[0]), (1 << 33) + 1], dtype=np.uint64))) == _capi.VK_EINVAL
    assert run(ws_bytes=int(ws_bytes.value) - 1) == _capi.VK_EINVAL
    torch.cuda.synchronize()
    # the engine's own refusals
    with pytest.raises(ValueError):
        eng.spectrum_fasta(dev, offs, lens, k=15)
    with pytest.raises(ValueError):
        eng.spectrum_fasta(dev, offs, lens, every=0)
    with pytest.raises(ValueError):
        eng.spectrum_fasta(dev, offs, lens, sketch=(64, 2))
