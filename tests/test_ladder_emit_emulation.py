"""Step C's file kernels (csrc/vk_emit.h) compiled for the host (tests/emul/emit_emul.cpp) against
tests/ladder_emit_ref.py, byte for byte.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ladder_emit_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 0xAB


@pytest.fixture(scope="module")
def emul():
    src = os.path.join(HERE, "emul", "emit_emul.cpp")
    so = os.path.join(HERE, "emul", "libemit_emul.so")
    csrc = os.path.join(ROOT, "varkoder_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("vk_emit.h", "vk_lane.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", csrc, src, "-o", so])
    L = C.CDLL(so)
    u64p = C.POINTER(C.c_uint64)
    L.emul_emit.argtypes = [C.c_char_p, C.c_uint64, u64p, u64p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, u64p, u64p,
                            C.POINTER(C.c_uint32)]

    def run(text, steps, cap=None):
        """steps = [(seed, threshold, whole)] -> (return code, each step's text, status, the bytes behind cap)"""
        n = len(steps)
        seeds = (C.c_uint64 * n)(*[s[0] for s in steps])
        thr = (C.c_uint64 * n)(*[s[1] for s in steps])
        whole = bytes(int(bool(s[2])) for s in steps)
        room = (3 * len(text) + 64) * n if cap is None else cap
        out = np.full(room + 64, GUARD, dtype=np.uint8)
        offs, lens, st = (C.c_uint64 * n)(), (C.c_uint64 * n)(), C.c_uint32()
        rc = L.emul_emit(text, len(text), seeds, thr, whole, n, out.ctypes.data, room, offs, lens, C.byref(st))
        got = [out[offs[j]:offs[j] + lens[j]].tobytes() for j in range(n)] if rc == 0 else None
        return rc, got, st.value, out[room:]
    return run


STEPS = [(seed, thr, False) for seed in R.SEEDS for thr in R.THRESHOLDS] + [(3, 0, True)]


@pytest.mark.parametrize("k", [5, 6, 7, 8, 9])
def test_the_kernels_write_the_rules_bytes(emul, k):
    for name, text in R.case_inputs(k).items():
        rc, got, status, guard = emul(text, STEPS)
        assert rc == 0 and status == 0, name
        for step, body in zip(STEPS, got):
            assert body == R.emit_ref(text, *step), (name, step)
        assert (guard == GUARD).all(), name


def test_bad_framing_gets_the_read_indexs_status_and_no_text(emul):
    good = R.case_inputs(5)["lengths"]
    for text in (good[1:], good.replace(b"\n+\n", b"\n-\n", 1), good + b"@x\nAC\n", b"@r\nAC\n+\n", b"", b"@r\nAC\n+\nII"):
        rc, got, status, _ = emul(text, STEPS)
        assert rc == 0 and status == R.framing_status(text)
        assert got == [R.emit_ref(text, *step) for step in STEPS]
        assert bool(status) == (not any(got)) or not text


def test_a_buffer_one_byte_short_is_not_written(emul):
    text = R.case_inputs(7)["long_header"]
    steps = [(1, 1 << 32, False), (2, 0, True)]
    need = sum((len(R.emit_ref(text, *s)) + 15) // 16 * 16 for s in steps)
    rc, _, _, guard = emul(text, steps, cap=need - 1)
    assert rc == 6 and (guard == GUARD).all()
    rc, got, _, guard = emul(text, steps, cap=need)
    assert rc == 0 and got == [R.emit_ref(text, *s) for s in steps] and (guard == GUARD).all()
