"""vk_unpng_device on the GPU: the files of tests/unpng_cases.py, one call per side, with PIL's pixels as the judge (the
cases and the numpy reference stand on PIL: tests/test_unpng_ref.py; the un-filter's arithmetic also runs on the host:
tests/test_unpng_emulation.py).  What only the GPU has is checked here: the inflate kernel on zlib streams, the phases'
barriers, lanes that run in any order, the C entry point's checks, damaged streams between good ones."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import png_cases as P
import unpng_cases as U
from varkoder_amd import _capi, pngread as R

pytestmark = pytest.mark.gpu

GUARD, PAD = 0xAB, 64
BAD_STREAM, TRUNCATED, BAD_SIZE, BAD_ADLER, BAD_FILTER = 1, 2, 4, 8, 16


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def laid_out(streams, side):
    """(buffer, offsets, lengths) of zlib streams as include/vkimg.h states it"""
    offs, lens, total = R.stream_layout([len(s) for s in streams])
    buf = np.zeros(total, dtype=np.uint8)
    for s, o in zip(streams, offs):
        buf[int(o):int(o) + len(s) + 4] = np.frombuffer(s + struct.pack("<I", side * (side + 1)), dtype=np.uint8)
    return buf, offs, lens


def call(eng, streams, side, change=None):
    """vk_unpng_device on zlib streams with guard bytes around d_img: (return code, images [n, side, side], statuses,
    the guard bytes, the whole d_img buffer).  change: arguments replaced (the EINVAL cases)."""
    import torch
    n = len(streams)
    buf, offs, lens = laid_out(streams, side)
    ws = C.c_uint64()
    assert eng.L.vk_unpng_workspace_size(min(max(side, 1), 512), max(n, 1), C.byref(ws)) == 0
    dev = torch.from_numpy(buf).to(eng.device)
    out = torch.full((PAD + n * side * side + PAD,), GUARD, dtype=torch.uint8, device=eng.device)
    wk = torch.empty(max(ws.value, 256), dtype=torch.uint8, device=eng.device)
    status = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    a = dict(ctx=eng.ctx, d_streams=C.c_void_p(dev.data_ptr()), offs=_u64(offs), lens=_u64(lens), n=n, side=side,
             img=C.c_void_p(out.data_ptr() + PAD), status=status.ctypes.data_as(C.POINTER(C.c_uint32)), wk=C.c_void_p(wk.data_ptr()),
             wb=ws.value)
    change = dict(change or {})
    if "offs_values" in change:
        offs = np.asarray(change.pop("offs_values"), dtype=np.uint64)
        a["offs"] = _u64(offs)
    if "lens_values" in change:
        lens = np.asarray(change.pop("lens_values"), dtype=np.uint64)
        a["lens"] = _u64(lens)
    a.update(change)
    rc = eng.L.vk_unpng_device(a["ctx"], a["d_streams"], a["offs"], a["lens"], a["n"], a["side"], a["img"], a["status"], a["wk"], a["wb"])
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    img = host[PAD:PAD + n * side * side].reshape(n, side, side)
    return rc, img, status, np.concatenate([host[:PAD], host[PAD + n * side * side:]]), host


@pytest.fixture(scope="module")
def eng(engines):
    return engines(7)


@pytest.mark.parametrize("side", sorted(set(P.SIDES) | set(U.EXTRA_SIDES)))
def test_every_case_of_a_side_in_one_call(eng, side):
    items = U.by_side()[side]
    rc, img, status, guard, _ = call(eng, [U.stream_of(d) for _, d, _ in items], side)
    assert rc == 0 and (guard == GUARD).all()
    assert not status.any(), [(n, int(s)) for (n, _, _), s in zip(items, status) if s]
    wrong = [n for (n, _, a), got in zip(items, img) if not (got == a).all()]
    assert not wrong, wrong


@pytest.mark.parametrize("side", [32, 256, 512])
def test_round_trip_with_the_encoder(eng, side):
    import torch
    arrs = np.stack([a for _, a in P.by_side()[side]])
    dev = torch.from_numpy(arrs).to(eng.device)
    chunks = eng.png(dev)
    streams = [c[8:-4] for c in chunks]
    back, status = eng.unpng(laid_out(streams, side), side)
    assert not status.any() and back.dtype == torch.uint8 and tuple(back.shape) == arrs.shape
    assert torch.equal(back, dev)


def test_one_image_and_two_thousand_of_side_32_in_one_call(eng):
    items = U.by_side()[32]
    streams = [U.stream_of(d) for _, d, _ in items]
    rc, img, status, guard, _ = call(eng, streams[3:4], 32)
    assert rc == 0 and list(status) == [0] and (guard == GUARD).all() and (img[0] == items[3][2]).all()
    idx = [(i * 5 + i // len(items)) % len(items) for i in range(2000)]   # (neighbours differ)
    rc, img, status, guard, _ = call(eng, [streams[j] for j in idx], 32)
    assert rc == 0 and not status.any() and (guard == GUARD).all()
    assert (img == np.stack([items[j][2] for j in idx])).all()


def test_the_engine_method_across_its_call_budget(eng, monkeypatch):
    from varkoder_amd import engine as E
    items = U.by_side()[65]
    datas, parts = [d for _, d, _ in items], [R.png_parts(d) for _, d, _ in items]
    want = np.stack([a for _, _, a in items])
    streams = R.pack_streams(datas, parts, 65)
    img, status = eng.unpng(streams, 65)
    assert not status.any() and (img.cpu().numpy() == want).all()
    ws = C.c_uint64()
    eng.L.vk_unpng_workspace_size(65, 1, C.byref(ws))
    with monkeypatch.context() as m:
        m.setattr(E, "PNG_CALL_BYTES", 3 * (ws.value + 64) + 3000)   # a few images a call
        img, status = eng.unpng(streams, 65)
        assert not status.any() and (img.cpu().numpy() == want).all()
        m.setattr(E, "PNG_CALL_BYTES", 1)   # below one image: one image a call
        img, status = eng.unpng((streams[0], streams[1][:4], streams[2][:4]), 65)
        assert not status.any() and (img.cpu().numpy() == want[:4]).all()
    img, status = eng.unpng((streams[0], streams[1][:0], streams[2][:0]), 65)
    assert tuple(img.shape) == (0, 65, 65) and len(status) == 0


def damaged(side, arr):
    """name -> (zlib stream, the bits it may get, the bits it must not get)"""
    raw = U.filtered(arr, "mix")
    stored, coded = U.deflated(raw, "stored"), U.deflated(raw, "level9")
    adler = struct.pack(">I", zlib.adler32(raw))
    bad_filter = bytearray(raw)
    bad_filter[(side - 1) * (side + 1)] = 5
    flipped = bytearray(coded)
    flipped[-2] ^= 0x10
    every = BAD_STREAM | TRUNCATED | BAD_SIZE | BAD_ADLER | BAD_FILTER
    return {
        "cut_in_a_stored_block": (stored[:len(stored) // 2], TRUNCATED, every ^ TRUNCATED),
        # (cut in a coded block, the four length bytes are read as codes before the input ends: either bit, no other)
        "cut_in_a_coded_block": (coded[:len(coded) // 2], TRUNCATED | BAD_STREAM, every ^ (TRUNCATED | BAD_STREAM)),
        "block_type_3": (coded[:2] + b"\x07" + adler, BAD_STREAM, every ^ BAD_STREAM),
        "stored_bad_nlen": (stored[:2] + b"\x01\x10\x00\xee\xff" + raw[:16] + adler, BAD_STREAM, every ^ BAD_STREAM),
        "too_long_coded": (U.deflated(raw + bytes(10), "level9"), BAD_SIZE, every ^ BAD_SIZE),
        "too_long_stored": (U.deflated(raw + bytes(10), "stored"), BAD_SIZE, every ^ BAD_SIZE),
        "too_short": (U.deflated(raw[:-5], "level9"), BAD_SIZE, every ^ BAD_SIZE),
        "adler_flipped": (bytes(flipped), BAD_ADLER, every ^ BAD_ADLER),
        "filter_byte_5": (U.deflated(bytes(bad_filter), "level9"), BAD_FILTER, every ^ BAD_FILTER),
    }


@pytest.mark.parametrize("side", [65, 130])
def test_damaged_streams_get_their_bit_between_two_good_images(eng, side):
    """In the manner of test_inflate_flags_bad_streams_and_never_writes_past_its_slot: good, bad, good, bad, ..., good.
    Every bad stream gets its bit, every good neighbour decodes right, the bytes around d_img are intact."""
    imgs = U.images()
    good = [(U.stream_of(U.forced(imgs[f"s{side}_{kind}"], mode, flavour)), imgs[f"s{side}_{kind}"])
            for kind, mode, flavour in (("levels7", 4, "level9"), ("uniform", 3, "stored"), ("smooth", "mix", "level1"))]
    bad = damaged(side, imgs[f"s{side}_levels7"])
    streams, wants = [good[0][0]], [good[0][1]]
    for i, (name, (stream, may, must_not)) in enumerate(bad.items()):
        streams += [stream, good[(i + 1) % 3][0]]
        wants += [None, good[(i + 1) % 3][1]]
    rc, img, status, guard, _ = call(eng, streams, side)
    assert rc == 0 and (guard == GUARD).all()
    print([(n, int(s)) for n, s in zip(bad, status[1::2])])
    for i, (name, (stream, may, must_not)) in enumerate(bad.items()):
        st = int(status[1 + 2 * i])
        assert st & may and not st & must_not, (name, st)
    for j in range(0, len(streams), 2):
        assert status[j] == 0 and (img[j] == wants[j]).all(), j


def test_every_einval_leaves_d_img_untouched(eng):
    side = 64
    items = U.by_side()[side][:4]
    streams = [U.stream_of(d) for _, d, _ in items]
    _, offs, lens = laid_out(streams, side)
    rc, img, status, guard, _ = call(eng, streams, side)
    assert rc == 0 and not status.any()
    ws = C.c_uint64()
    eng.L.vk_unpng_workspace_size(side, 4, C.byref(ws))
    bad_off, short = offs.copy(), lens.copy()
    bad_off[2] += 8
    short[1] = 9
    for change in (dict(ctx=None), dict(d_streams=None), dict(offs=None), dict(lens=None), dict(img=None), dict(status=None),
                   dict(wk=None), dict(n=0), dict(side=0), dict(side=513), dict(offs_values=bad_off), dict(lens_values=short),
                   dict(wb=ws.value - 1)):
        what = dict(change)
        rc, _, status, _, host = call(eng, streams, side, change)
        assert rc == _capi.VK_EINVAL, what
        assert (host == GUARD).all() and (status == 0xFFFFFFFF).all(), what
    short[1] = 10   # 2 + 4 + 4: the shortest length taken (nothing to inflate: a status, not an error)
    rc, _, status, guard, _ = call(eng, streams, side, dict(lens_values=short))
    assert rc == 0 and status[1] != 0 and status[0] == 0 and (guard == GUARD).all()
