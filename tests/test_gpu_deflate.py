"""vk_deflate_device on the GPU: one call over every text of tests/deflate_cases.py, with zlib as the judge
(gzip.decompress and zlib.decompressobj(31), member by member), then the product's own reader.

The size checks (deflate_cases.check_file): every member of the FASTQ-shaped and skewed texts is no larger than zlib's
Huffman-only block of the same text + 286 bytes of table allowance + 26 of framing, and every member of the
repeated-record text is under half of that Huffman-only size (the text is 60,000 bytes, one member, and the check is
asked of it).  Whether zlib level 1 itself meets the two conditions on these inputs was checked on the CPU
(asserted in tests/test_deflate_emulation.py): it meets both on every FASTQ-shaped text and on the repeated record, and does NOT meet the first on the skewed text (20,011 bytes against
15,207 + 286 + 26): greedy matches in shuffled bytes cost more than the literals they replace.  The compressor here
meets it because it also prices the block of literals alone and writes the smaller one."""
import ctypes as C

import numpy as np
import pytest

import deflate_cases as D

pytestmark = pytest.mark.gpu

GUARD = 0xAB


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _call(eng, dev, offs, lens, cap=None, fill=GUARD):
    """vk_deflate_device with a guarded output buffer: (status, whole buffer on the host, offsets, lengths, bound)"""
    import torch
    n = len(offs)
    bound, ws = C.c_uint64(), C.c_uint64()
    assert eng.L.vk_deflate_bound(_u64(lens), n, C.byref(bound)) == 0
    assert eng.L.vk_deflate_workspace_size(_u64(lens), n, C.byref(ws)) == 0
    cap = bound.value if cap is None else cap
    out = torch.full((bound.value + 64,), fill, dtype=torch.uint8, device=eng.device)
    work = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=eng.device)
    oo, ol = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    st = eng.L.vk_deflate_device(eng.ctx, C.c_void_p(dev.data_ptr()), _u64(offs), _u64(lens), n, C.c_void_p(out.data_ptr()), cap,
                                 C.c_void_p(work.data_ptr()), work.numel(), _u64(oo), _u64(ol))
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), oo, ol, bound.value


@pytest.fixture(scope="module")
def batch(engines):
    eng = engines(7)
    named = list(D.texts().items()) + [(f"small_{i}", t) for i, t in enumerate(D.small_files())]
    dev, offs, lens = eng.upload([t for _, t in named])
    st, host, oo, ol, bound = _call(eng, dev, offs, lens)
    assert st == 0
    files = [host[int(o):int(o + n)].tobytes() for o, n in zip(oo, ol)]
    return eng, named, (dev, offs, lens), host, oo, ol, bound, files


def test_every_file_inflates_to_its_text_and_is_bgzf(batch):
    from varkoder_amd import engine as E
    eng, named, _, host, oo, ol, bound, files = batch
    assert (oo % 16 == 0).all() and int(oo[-1] + ol[-1]) <= bound
    assert all(int(oo[i] + ol[i]) <= int(oo[i + 1]) for i in range(len(oo) - 1))
    for (name, text), data in zip(named, files):
        D.check_file(name, text, data)
        assert E.bgzf_members(data) is not None and E.bgzf_text_size(data) == len(text), name
    assert (host[bound:] == GUARD).all(), "bytes behind the bound were written"


def test_a_second_call_gives_the_same_bytes(batch):
    eng, named, (dev, offs, lens), _, oo, ol, _, files = batch
    st, host, oo2, ol2, _ = _call(eng, dev, offs, lens)
    assert st == 0 and (oo2 == oo).all() and (ol2 == ol).all()
    assert [host[int(o):int(o + n)].tobytes() for o, n in zip(oo2, ol2)] == files


def test_the_engine_method_and_the_products_own_reader(batch, tmp_path):
    eng, named, (dev, offs, lens), _, oo, ol, _, files = batch
    out, o2, l2 = eng.deflate(dev, offs, lens)
    got = out[:int(o2[-1] + l2[-1])].cpu().numpy()
    assert [got[int(o):int(o + n)].tobytes() for o, n in zip(o2, l2)] == files
    pick = [i for i, (name, _) in enumerate(named) if not name.startswith("small_") or i % 25 == 0]
    paths = []
    for i in pick:
        p = tmp_path / f"f{i}.fq.gz"
        p.write_bytes(files[i])
        paths.append(p)
    text, toffs, tlens = eng.upload_files(paths)[:3]
    host = text.cpu().numpy()
    for i, o, n in zip(pick, toffs, tlens):
        assert host[int(o):int(o + n)].tobytes() == named[i][1], named[i][0]


def test_errors_are_found_before_anything_is_written(batch):
    from varkoder_amd import _capi
    eng, named, (dev, offs, lens), _, _, _, bound, _ = batch
    bad = offs.copy()
    bad[1] += 8
    st, host, _, _, _ = _call(eng, dev, bad, lens)
    assert st == _capi.VK_EINVAL and (host == GUARD).all()
    st, host, _, _, _ = _call(eng, dev, offs, lens, cap=bound - 1)
    assert st == _capi.VK_ENOSPC and (host == GUARD).all()
    b = C.c_uint64()
    assert eng.L.vk_deflate_bound(None, 3, C.byref(b)) == _capi.VK_EINVAL
    assert eng.L.vk_deflate_device(eng.ctx, None, _u64(offs), _u64(lens), len(offs), None, 0, None, 0, None, None) == _capi.VK_EINVAL
