#!/usr/bin/env python3
"""The sketches (vk_sketch_device, vk_sketch_pairs_device: `--spectrum-sketch`, `distance`) beside the spectrum they are
taken from.

Selection: 2 x --pairs synthetic reads of --len bases with 0.5 % substitutions, both strands, from a genome large enough
for 0.3x (nearly every window a new key), as one cleaned FASTQ text in HBM, counted at K = 21 with every = 1 and 16 into
the engine's tables; then, on those tables, vk_sketch_device with s = 16,384 and 2^20 (min_count 1).  Prints per run the
time of the whole vk_spectrum_device call and of the vk_sketch_device call (best of --reps, each between two device
synchronisations, buffers allocated before), the table's slots, bytes and load, and the ratio.  The parent's kernels
vk_sp_count_kernel and vk_sp_hist_kernel are the yardstick: under `rocprofv3 --kernel-trace --stats -- python
tools/sketch_time.py --reps 1 --no-pairs` their times and those of the vk_sk_* kernels come from the trace.

Pairs: --sketches sketches of 16,384 hashes drawn from a common pool (so that they overlap), every pair by one
vk_sketch_pairs_device call (the call between two synchronisations, and ImageEngine.sketch_pairs with its copies), beside
the NumPy route on the host (np.union1d, np.intersect1d, np.isin per pair) for the same answers on --host-pairs of them,
scaled to all.

usage: python tools/sketch_time.py [--pairs N] [--len L] [--reps R] [--sketches N] [--host-pairs N] [--no-pairs] [--no-select]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from spectrum_time import fastq_of, reads_of  # noqa: E402


def u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sketches", type=int, default=512)
    ap.add_argument("--host-pairs", type=int, default=512)
    ap.add_argument("--no-pairs", action="store_true")
    ap.add_argument("--no-select", action="store_true")
    a = ap.parse_args()
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    L, p = eng.L, eng._ptr

    def sync():
        _capi.check(eng.ctx, L.vk_ctx_sync(eng.ctx), "vk_ctx_sync")
        torch.cuda.synchronize()

    def best(call):
        out = []
        for _ in range(a.reps):
            sync()
            t = time.perf_counter()
            call()
            sync()
            out.append(time.perf_counter() - t)
        return min(out)

    if not a.no_select:
        n, rl = 2 * a.pairs, a.len
        rng = np.random.default_rng(7)
        reads = reads_of(rng, int(n * rl / 0.3), n, rl)
        dev, offs, lens = eng.upload([fastq_of(reads)])
        recs = np.array([n], dtype=np.uint64)
        print(f"# selection: {n} reads x {rl} bp, 0.5 % substitutions, 0.3x, K 21, text {int(lens[0])} bytes, best of {a.reps}; times in ms")
        for every in (1, 16):
            nsl = np.array([eng.spectrum_slots(int(lens[0]), every)], dtype=np.uint64)
            base = np.zeros(1, dtype=np.uint64)
            keys = torch.empty(int(nsl[0]), dtype=torch.int64, device=eng.device)
            counts = torch.empty(int(nsl[0]), dtype=torch.int32, device=eng.device)
            wsb = C.c_uint64()
            _capi.check(eng.ctx, L.vk_spectrum_workspace_size(u64(recs), 1, u64(lens), C.byref(wsb)), "vk_spectrum_workspace_size")
            ws = torch.empty(int(wsb.value), dtype=torch.uint8, device=eng.device)
            rows = torch.empty((1, _capi.VK_SPEC_NSTAT), dtype=torch.int64, device=eng.device)
            status = torch.empty(1, dtype=torch.int32, device=eng.device)

            def spectrum():
                _capi.check(eng.ctx, L.vk_spectrum_device(eng.ctx, p(dev), u64(offs), u64(lens), u64(recs), 1, 21, every, p(keys),
                                                          p(counts), u64(base), u64(nsl), p(rows), p(status), p(ws), ws.numel()),
                            "vk_spectrum_device")
            t_spec = best(spectrum)
            assert int(status.cpu()[0]) == 0
            distinct = int(rows.cpu().numpy().view(np.uint64)[0, 4])
            print(f"every {every:2d}: table {int(nsl[0])} slots, {int(nsl[0]) * 12 / 2**20:.0f} MiB, distinct {distinct}, load "
                  f"{distinct / int(nsl[0]):.3f}; vk_spectrum_device {t_spec * 1e3:9.2f}")
            for s in (16384, 1 << 20):
                _capi.check(eng.ctx, L.vk_sketch_workspace_size(u64(nsl), 1, s, C.byref(wsb)), "vk_sketch_workspace_size")
                sws = torch.empty(int(wsb.value), dtype=torch.uint8, device=eng.device)
                hashes = torch.empty((1, s), dtype=torch.int64, device=eng.device)
                info = torch.empty((1, 2), dtype=torch.int64, device=eng.device)

                def sketch():
                    _capi.check(eng.ctx, L.vk_sketch_device(eng.ctx, p(keys), p(counts), u64(base), u64(nsl), 1, p(status), 1, s,
                                                            p(hashes), p(info), p(sws), sws.numel()), "vk_sketch_device")
                t_sk = best(sketch)
                inf = info.cpu().numpy().view(np.uint64)[0]
                h = hashes.cpu().numpy().view(np.uint64)[0, :int(inf[1])]
                assert int(inf[0]) == distinct and (h[1:] > h[:-1]).all()
                print(f"    s {s:7d}: vk_sketch_device {t_sk * 1e3:8.2f}  length {int(inf[1])}  workspace {int(wsb.value) / 2**20:.1f} MiB  "
                      f"{int(nsl[0]) * 12 / t_sk / 1e9:7.1f} GB/s of one table pass  sketch / spectrum {t_sk / t_spec:6.3f}")
                del sws, hashes
            del keys, counts, ws
        del dev

    if not a.no_pairs:
        s, ns = 16384, a.sketches
        rng = np.random.default_rng(9)
        pool = np.unique(rng.integers(0, 2 ** 63, 3 * s, dtype=np.uint64))
        rows = np.stack([np.sort(rng.choice(pool, s, replace=False)) for _ in range(ns)])
        lens = np.full(ns, s, dtype=np.uint64)
        dq = torch.from_numpy(rows.view(np.int64)).to(eng.device)
        dl = torch.from_numpy(lens.view(np.int64)).to(eng.device)
        shared = torch.empty((ns, ns), dtype=torch.int32, device=eng.device)
        seen = torch.empty((ns, ns), dtype=torch.int32, device=eng.device)

        def pairs():
            _capi.check(eng.ctx, L.vk_sketch_pairs_device(eng.ctx, p(dq), p(dl), ns, p(dq), p(dl), ns, s, p(shared), p(seen)),
                        "vk_sketch_pairs_device")
        t_dev = best(pairs)
        t_eng = best(lambda: eng.sketch_pairs(rows, lens, rows, lens, s))
        sh, se = shared.cpu().numpy(), seen.cpu().numpy()
        m = min(a.host_pairs, ns * ns)
        t = time.perf_counter()
        host = [pair_numpy(rows[i // ns], rows[i % ns], s) for i in range(m)]
        t_host = time.perf_counter() - t
        assert host == [(int(sh[i // ns, i % ns]), int(se[i // ns, i % ns])) for i in range(m)]
        print(f"# pairs: {ns} sketches of {s}, {ns * ns} pairs; times in ms")
        print(f"vk_sketch_pairs_device {t_dev * 1e3:9.2f} ({ns * ns / t_dev / 1e6:.2f} M pairs/s)  ImageEngine.sketch_pairs with its copies "
              f"{t_eng * 1e3:9.2f}  NumPy on the host {t_host * 1e3:9.2f} for {m} pairs = {t_host / m * ns * ns * 1e3:.0f} for all "
              f"({t_host / m * ns * ns / t_dev:.0f} x the device call)")
    eng.close()


def pair_numpy(sa, sb, s):
    union = np.union1d(sa, sb)[:s]
    both = np.intersect1d(sa, sb, assume_unique=True)
    return int(np.isin(union, both, assume_unique=True).sum()), int(len(union))


if __name__ == "__main__":
    main()
