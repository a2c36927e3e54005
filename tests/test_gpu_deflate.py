"""vk_deflate_device on the GPU: one call over every text of tests/deflate_cases.py, with zlib as the judge
(gzip.decompress and zlib.decompressobj(31), member by member), then the product's own reader.

The size checks (deflate_cases.check_file): every member of the FASTQ-shaped and skewed texts is no larger than zlib's
Huffman-only block of the same text + 286 bytes of table allowance + 26 of framing, and every member of the
repeated-record text is under half of that Huffman-only size (the text is 60,000 bytes, one member, and the check is
asked of it).  Whether zlib level 1 itself meets the two conditions on these inputs was checked on the CPU
(asserted in tests/test_deflate_emulation.py): it meets both on every FASTQ-shaped text and on the repeated record, and does NOT meet the first on the skewed text (20,011 bytes against
15,207 + 286 + 26): greedy matches in shuffled bytes cost more than the literals they replace.  The compressor here
meets it because it also prices the block of literals alone and writes the smaller one.

The GPU's bytes are also the host emulation's bytes (tests/emul/deflate_emul.cpp: the same csrc/vk_deflate.h, its lanes run
one after another): tests/golden/deflate_sweep_sha256.json records the emulation's files, tests/test_deflate_emulation.py
keeps the record true, and the tests here compare every file's sha256 with it.  That is the check of what only the GPU
has -- barriers between the phases, LDS atomics, lanes that run in any order, the gather kernel, the scans."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import deflate_cases as D

pytestmark = pytest.mark.gpu

GUARD = 0xAB


@pytest.fixture(scope="module")
def recorded():
    with open(D.DIGESTS) as f:
        return json.load(f)


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def _files(host, oo, ol):
    return [host[int(o):int(o + n)].tobytes() for o, n in zip(oo, ol)]


def _layout_is_packed(host, oo, ol, bound):
    """Files at multiples of 16, ascending, not overlapping, zero bytes from a file's end to the next file, nothing
    written behind the bound."""
    assert (oo % 16 == 0).all() and int(oo[-1] + ol[-1]) <= bound
    ends = (oo + ol).astype(np.int64)
    assert (ends[:-1] <= oo[1:].astype(np.int64)).all() and (oo[1:].astype(np.int64) - ends[:-1] < 16).all()
    for e, o in zip(ends[:-1], oo[1:]):
        assert not host[int(e):int(o)].any(), "bytes between two files are not zero"
    assert (host[bound:] == GUARD).all(), "bytes behind the bound were written"


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


def test_the_fixed_list_gives_the_emulations_bytes(batch, recorded):
    _, named, _, _, _, _, _, files = batch
    for (name, _), data in zip(named, files):
        assert _sha(data) == recorded[name], name


def test_the_sweep_in_one_call_gives_the_emulations_bytes(engines, recorded):
    """Every text of deflate_cases.sweep() (periods, every match length, every distance symbol's edges, 1,100 prefix
    lengths, alphabets of one, two and 256 values, codes at the 15-bit limit, a match over a whole round, 300 seeded
    fuzz texts), one call.  Each file passes check_file and is, byte for byte, the file that the host emulation writes."""
    eng = engines(7)
    named = list(D.sweep().items())
    dev, offs, lens = eng.upload([t for _, t in named])
    st, host, oo, ol, bound = _call(eng, dev, offs, lens)
    assert st == 0
    _layout_is_packed(host, oo, ol, bound)
    differ = []
    for (name, text), data in zip(named, _files(host, oo, ol)):
        D.check_file(name, text, data)
        if _sha(data) != recorded[name]:
            differ.append(name)
    assert not differ, differ


def test_the_gather_writes_members_at_every_alignment(engines, recorded):
    """40 files of 3..5 members: the places of the non-first members in their files have every residue mod 4 at least 8
    times (asserted on the emulation's sizes in tests/test_deflate_emulation.py; the sizes here are the same, the
    digests say), so vk_df_gather_kernel's lead bytes, realigned dwords and tail bytes all run, from slots whose
    members have every length mod 4."""
    eng = engines(7)
    texts = D.gather_files()
    dev, offs, lens = eng.upload(texts)
    st, host, oo, ol, bound = _call(eng, dev, offs, lens)
    assert st == 0
    _layout_is_packed(host, oo, ol, bound)
    residues = [0, 0, 0, 0]
    for i, (text, data) in enumerate(zip(texts, _files(host, oo, ol))):
        assert _sha(data) == recorded[f"gather_{i}"], i
        D.check_file(f"gather_{i}", text, data)
        at = 0
        for j, (member, _) in enumerate(D.members_of(data)[:-1]):
            residues[at % 4] += j > 0
            at += len(member)
    assert min(residues) >= 8, residues


def test_scans_over_more_than_one_block(engines, recorded):
    """9,000 files and 7,604 members in one call: both prefix sums of vk_deflate_device take more than one block of
    4,096 (two for the members, three for the files, through one `sums` buffer), with fewer members than files among
    the first 4,200 files, a file whose five members lie on both sides of member 4096, and files around file 4096 whose
    sizes are no multiples of 16.  The engine's method is held against the C call's bytes on this batch."""
    eng = engines(7)
    texts = D.scan_files()
    D.check_scan_batch(texts)
    dev, offs, lens = eng.upload(texts)
    st, host, oo, ol, bound = _call(eng, dev, offs, lens)
    assert st == 0
    _layout_is_packed(host, oo, ol, bound)
    files = _files(host, oo, ol)
    D.check_scan_batch(texts, files)
    for i, (text, data) in enumerate(zip(texts, files)):
        D.check_file(f"scan_{i}", text, data)
    assert _sha(b"".join(files)) == recorded["scan_batch"]
    st, host2, oo2, ol2, _ = _call(eng, dev, offs, lens)
    assert st == 0 and (oo2 == oo).all() and (ol2 == ol).all()
    end = int(oo[-1] + ol[-1])
    assert (host2[:end] == host[:end]).all(), "a second call gives other bytes"
    out, o3, l3 = eng.deflate(dev, offs, lens)
    assert (o3 == oo).all() and (l3 == ol).all() and (out[:end].cpu().numpy() == host[:end]).all()
