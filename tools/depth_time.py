#!/usr/bin/env python3
"""The depth filter (vk_depth_device, ImageEngine.depth_filter: `--kmer-spectrum --depth-filter`) beside the spectrum's
count on the same text in the same run, on tools/spectrum_time.py's synthetic samples -- 2 x --pairs reads of --len bases
with 0.5 % substitutions, both strands, one cleaned FASTQ text in HBM:

  shallow   reads from a random genome large enough for 0.3x: nearly every probe ends at another cache line, depth 1
  deep      reads from a genome small enough for 30x: nearly every probe re-hits a key
  poly-A    the deep reads with a quarter replaced, half by poly-A and half by (ACGT)n: whole waves on one histogram bin

at K = 21, every = 1.  Per sample: the tables counted once (vk_spectrum_device, timed), then ImageEngine.depth_filter
against them with VKIMG_DEPTH_MERGE = 0 and 1 (how the match kernel adds to its LDS histogram), best of --reps,
device-synchronised: the read index, the match kernel, the scan, the copy of the kept records and the rows' copy.
Under `rocprofv3 --kernel-trace --stats -- python tools/depth_time.py --reps 1 --one NAME` the per-kernel times come
from the trace: vk_dp_match_kernel beside vk_sp_count_kernel.

Every sample runs in a child process of its own under its own time limit (--limit seconds); the first that fails or
runs out of time ends the tool.

usage: python tools/depth_time.py [--pairs N] [--len L] [--reps R] [--limit S] [--one shallow|deep|poly-A]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NAMES = ("shallow", "deep", "poly-A")
K, BAND = 21, (2, 2 ** 32 - 1)


def reads_for(name, n, L):
    from spectrum_time import ACGT, reads_of
    rng = np.random.default_rng(7)
    bases = n * L
    if name == "shallow":
        return reads_of(rng, int(bases / 0.3), n, L)
    reads = reads_of(rng, bases // 30, n, L)
    if name == "poly-A":
        reads[0::8] = ord("A")
        reads[4::8] = np.resize(ACGT, L)
    return reads


def one(name, a):
    import torch
    from spectrum_time import fastq_of
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine, _u64
    sync = torch.cuda.synchronize
    n, L = 2 * a.pairs, a.len

    def engine(merge):
        old = os.environ.pop("VKIMG_DEPTH_MERGE", None)
        os.environ["VKIMG_DEPTH_MERGE"] = str(merge)
        try:
            return ImageEngine(k=7, mapping="cgr", device=0)
        finally:
            os.environ.pop("VKIMG_DEPTH_MERGE", None)
            if old is not None:
                os.environ["VKIMG_DEPTH_MERGE"] = old

    engines = {m: engine(m) for m in (0, 1)}
    eng = engines[1]
    dev, offs, lens = eng.upload([fastq_of(reads_for(name, n, L))])
    recs = np.array([n], dtype=np.uint64)
    nsl = np.array([eng.spectrum_slots(int(lens[0]), 1)], dtype=np.uint64)
    base = np.zeros(1, dtype=np.uint64)
    keys = torch.empty(int(nsl[0]), dtype=torch.int64, device=eng.device)
    counts = torch.empty(int(nsl[0]), dtype=torch.int32, device=eng.device)
    ws_bytes = C.c_uint64()
    _capi.check(eng.ctx, eng.L.vk_spectrum_workspace_size(_u64(recs), 1, _u64(lens), C.byref(ws_bytes)), "vk_spectrum_workspace_size")
    ws = torch.empty(max(int(ws_bytes.value), 256), dtype=torch.uint8, device=eng.device)
    d_rows = torch.empty((1, _capi.VK_SPEC_NSTAT), dtype=torch.int64, device=eng.device)
    d_status = torch.empty(1, dtype=torch.int32, device=eng.device)
    spec = []
    for _ in range(a.reps):
        sync()
        t = time.perf_counter()
        st = eng.L.vk_spectrum_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), _u64(recs), 1, K, 1, eng._ptr(keys),
                                      eng._ptr(counts), _u64(base), _u64(nsl), eng._ptr(d_rows), eng._ptr(d_status), eng._ptr(ws),
                                      ws.numel())
        _capi.check(eng.ctx, st, "vk_spectrum_device")
        sync()
        spec.append(time.perf_counter() - t)
    row = d_rows.cpu().numpy().view(np.uint64)[0]
    assert int(d_status.cpu()[0]) == 0
    out = torch.empty((int(lens[0]) + 15) // 16 * 16 + 16, dtype=torch.uint8, device=eng.device)
    print(f"{name}: text {int(lens[0])} bytes, table {int(nsl[0])} slots load {int(row[4]) / int(nsl[0]):.3f}, windows {int(row[2])}; "
          f"vk_spectrum_device {min(spec) * 1e3:8.2f}", flush=True)
    for merge, e in engines.items():
        best = []
        for _ in range(a.reps):
            sync()
            t = time.perf_counter()
            olens, rows, status = e.depth_filter(dev, offs, lens, keys, counts, base, nsl, d_status, [BAND[0]], [BAND[1]], K, 1,
                                                 recs, out, [0])   # (waits for the kernels)
            best.append(time.perf_counter() - t)
        assert not status.any() and int(rows[0, 0]) == n
        print(f"  VKIMG_DEPTH_MERGE {merge}: depth_filter {min(best) * 1e3:8.2f}  ({int(row[2]) / min(best) / 1e9:5.2f} G windows/s, "
              f"{min(best) / min(spec):5.2f} x the spectrum call)  band {BAND[0]}: kept {int(rows[0, 1])} of {n} reads, {int(olens[0])} bytes; "
              f"median depth 0 / 1 / 2..254 / 255+: {int(rows[0, 5])} / {int(rows[0, 6])} / {int(rows[0, 7:260].sum())} / {int(rows[0, 260])}",
              flush=True)
    for e in engines.values():
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--one", choices=NAMES)
    a = ap.parse_args()
    if a.one:
        return one(a.one, a)
    print(f"# {2 * a.pairs} reads x {a.len} bp ({a.pairs} pairs), 0.5 % substitutions, K {K}, every 1, best of {a.reps}; times in ms",
          flush=True)
    for name in NAMES:   # (a child each, under its own time limit; nothing more is started after one that fails)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--pairs", str(a.pairs), "--len", str(a.len),
                            "--reps", str(a.reps)], timeout=a.limit)
        if r.returncode:
            sys.exit(f"{name}: exit status {r.returncode}")


if __name__ == "__main__":
    main()
