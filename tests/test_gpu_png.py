"""vk_png_device on the GPU: one call per side over that side's images of tests/png_cases.py, with zlib as the judge.

The GPU's bytes are also the host emulation's bytes (tests/emul/png_emul.cpp: the same csrc/vk_png.h and vk_deflate.h,
the lanes run one after another): tests/golden/png_sweep_sha256.json records the emulation's chunks,
tests/test_png_emulation.py keeps the record true, and the tests here compare every chunk's sha256 with it.  That is the
check of what only the GPU has -- barriers between the phases, LDS atomics, lanes that run in any order, the image and
gather kernels, the scans.  The size conditions are asserted on the emulation's bytes (tests/test_png_emulation.py)."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import png_cases as P

pytestmark = pytest.mark.gpu

GUARD = 0xAB


@pytest.fixture(scope="module")
def recorded():
    with open(P.DIGESTS) as f:
        return json.load(f)


def _sha(data):
    return hashlib.sha256(data).hexdigest()


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _call(eng, dev, cap=None, work=None):
    """vk_png_device on a device tensor [n, side, side] with a guarded output buffer: (status, whole buffer on the host,
    offsets, lengths, bound)"""
    import torch
    n, side = int(dev.shape[0]), int(dev.shape[1])
    bound, ws = C.c_uint64(), C.c_uint64()
    assert eng.L.vk_png_bound(side, n, C.byref(bound)) == 0
    assert eng.L.vk_png_workspace_size(side, n, C.byref(ws)) == 0
    cap = bound.value if cap is None else cap
    out = torch.full((bound.value + 64,), GUARD, dtype=torch.uint8, device=eng.device)
    wbytes = ws.value if work is None else work
    wk = torch.empty(max(wbytes, 256), dtype=torch.uint8, device=eng.device)
    oo, ol = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    st = eng.L.vk_png_device(eng.ctx, C.c_void_p(dev.data_ptr()), n, side, C.c_void_p(out.data_ptr()), cap,
                             C.c_void_p(wk.data_ptr()), wbytes, _u64(oo), _u64(ol))
    torch.cuda.synchronize()
    return st, out.cpu().numpy(), oo, ol, bound.value


def _chunks(host, oo, ol):
    return [host[int(o):int(o + n)].tobytes() for o, n in zip(oo, ol)]


def _layout_is_packed(host, oo, ol, bound):
    """Chunks at multiples of 16, ascending, not overlapping, zero bytes from a chunk's end to the next, nothing written
    behind the bound."""
    assert (oo % 16 == 0).all() and oo[0] == 0 and int(oo[-1] + ol[-1]) <= bound
    ends = (oo + ol).astype(np.int64)
    assert (ends[:-1] <= oo[1:].astype(np.int64)).all() and (oo[1:].astype(np.int64) - ends[:-1] < 16).all()
    for e, o in zip(ends[:-1], oo[1:]):
        assert not host[int(e):int(o)].any(), "bytes between two chunks are not zero"
    assert (host[bound:] == GUARD).all(), "bytes behind the bound were written"


@pytest.fixture(scope="module")
def device_cases(engines):
    import torch
    eng = engines(7)
    return eng, {side: (items, torch.from_numpy(np.stack([a for _, a in items])).to(eng.device))
                 for side, items in P.by_side().items()}


@pytest.mark.parametrize("side", P.SIDES)
def test_one_call_per_side_gives_the_emulations_bytes_twice(device_cases, recorded, side):
    eng, cases = device_cases
    items, dev = cases[side]
    st, host, oo, ol, bound = _call(eng, dev)
    assert st == 0
    _layout_is_packed(host, oo, ol, bound)
    differ = []
    for (name, arr), chunk in zip(items, _chunks(host, oo, ol)):
        P.check_chunk(name, arr, chunk)
        if _sha(chunk) != recorded[name]:
            differ.append(name)
    assert not differ, differ
    st, host2, oo2, ol2, _ = _call(eng, dev)
    end = int(oo[-1] + ol[-1])
    assert st == 0 and (oo2 == oo).all() and (ol2 == ol).all() and (host2[:end] == host[:end]).all()


def test_three_thousand_small_images_run_the_scans(device_cases, recorded):
    """3,000 images of side 23 in one call (its 14 cases over and over, in an order in which neighbours differ): the two
    scans run over 3,000 sizes, no multiple of their 256 lanes, and the gather places 3,000 chunks of many lengths."""
    import torch
    eng, cases = device_cases
    items, dev = cases[23]
    idx = torch.tensor([(i * 5 + i // 14) % len(items) for i in range(3000)], device=eng.device)
    st, host, oo, ol, bound = _call(eng, dev[idx].contiguous())
    assert st == 0
    _layout_is_packed(host, oo, ol, bound)
    want = [recorded[items[int(j)][0]] for j in idx.cpu()]
    assert [_sha(c) for c in _chunks(host, oo, ol)] == want


def test_the_engine_method_across_its_call_budget(device_cases, recorded, monkeypatch):
    from varkoder_amd import engine as E
    eng, cases = device_cases
    for side in (46, 256):
        items, dev = cases[side]
        single = eng.png(dev)
        assert [_sha(c) for c in single] == [recorded[n] for n, _ in items]
        bound, ws = C.c_uint64(), C.c_uint64()
        eng.L.vk_png_bound(side, 1, C.byref(bound))
        eng.L.vk_png_workspace_size(side, 1, C.byref(ws))
        with monkeypatch.context() as m:
            m.setattr(E, "PNG_CALL_BYTES", 3 * (bound.value + ws.value) + 1)   # three images a call
            assert eng.png(dev) == single
            m.setattr(E, "PNG_CALL_BYTES", 1)   # below one image: one image a call
            assert eng.png(dev[:4]) == single[:4]
    assert eng.png(cases[46][1][:0]) == []


def test_errors_are_found_before_anything_is_written(device_cases):
    import torch
    from varkoder_amd import _capi
    eng, cases = device_cases
    _, dev = cases[64]
    n = int(dev.shape[0])
    st, host, _, _, bound = _call(eng, dev, cap=None)
    assert st == 0
    st, host, _, _, _ = _call(eng, dev, cap=bound - 1)
    assert st == _capi.VK_ENOSPC and (host == GUARD).all()
    ws = C.c_uint64()
    eng.L.vk_png_workspace_size(64, n, C.byref(ws))
    st, host, _, _, _ = _call(eng, dev, work=ws.value - 1)
    assert st == _capi.VK_EINVAL and (host == GUARD).all()
    out = torch.full((bound + 64,), GUARD, dtype=torch.uint8, device=eng.device)
    wk = torch.empty(ws.value, dtype=torch.uint8, device=eng.device)
    oo, ol = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    good = dict(ctx=eng.ctx, img=C.c_void_p(dev.data_ptr()), n=n, side=64, out=C.c_void_p(out.data_ptr()), cap=bound,
                wk=C.c_void_p(wk.data_ptr()), wb=ws.value, oo=_u64(oo), ol=_u64(ol))
    for change in (dict(ctx=None), dict(img=None), dict(out=None), dict(wk=None), dict(oo=None), dict(ol=None), dict(n=0),
                   dict(side=0), dict(side=513)):
        a = dict(good, **change)
        st = eng.L.vk_png_device(a["ctx"], a["img"], a["n"], a["side"], a["out"], a["cap"], a["wk"], a["wb"], a["oo"], a["ol"])
        assert st == _capi.VK_EINVAL, change
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()
