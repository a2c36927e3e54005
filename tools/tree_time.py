#!/usr/bin/env python3
"""`tree`'s call (vk_tree_nj_device, ImageEngine.nj_device) beside the rule's NumPy statement (tests/tree_ref.py, nj_np) on
the host: one tree of 256, 1,024 and 4,096 leaves and 101 trees of 256 leaves in one call (a main tree and 100 replicates).
The matrices hold the distances between random points of a cube.  The device's time is the synchronised wall time of the call on
a matrix already in HBM, best of --reps after a warm-up; the reference is timed once, for 4,096 leaves on its first --sample
steps and scaled by the steps' share of the whole run's entries (a step of m slots costs m^2); of the 101 trees five are
timed and the sum is scaled.

Then the search launch alone (vk_tree_search_probe_device): calls of 4 and of 4 + --launches search launches, the
difference over --launches, against the bytes a search of n active slots must read -- the upper triangle, 8 n (n - 1) / 2
-- as a share of the 8.0 TB/s HBM peak and of the 6.29 TB/s a float4 copy reaches.  A matrix of up to 4,096
leaves (134 MB) stays in the 256 MB Infinity Cache from one launch to the next, as it does from one step to the next in a real
call, so the figure there is the cache's; 8,192 leaves (537 MB) do not fit, and that row is HBM's.

Last, what a call spends between launches: --trace N runs three calls of N leaves and nothing else, for
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/tree_time.py --trace N`;
--stats DIR/..._kernel_stats.csv --wall MS then prints the kernels' summed time per call and the rest's share of the wall time.

usage: python tools/tree_time.py [--reps R] [--sample S] [--launches L] [--skip-reference] | --trace N | --stats CSV --wall MS
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))   # (tree_ref: the rule's NumPy statement)

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def matrix(n, seed):
    """Distances between n random points of an 8-dimensional cube: symmetric bit for bit, the diagonal 0, and made in
    O(n^2) NumPy operations whatever n."""
    x = np.random.default_rng(seed).random((n, 8))
    d = np.zeros((n, n))
    for c in range(8):
        diff = x[:, c][:, None] - x[:, c][None, :]
        d += diff * diff
    return np.sqrt(d)


def device_time(eng, torch, d, reps):
    """Best synchronised wall time of a call on a fresh device copy of d [ntrees, n, n]; the last call's outputs."""
    times = []
    src = torch.from_numpy(d).to(eng.device)
    for rep in range(reps + 1):   # (the first warms up)
        dd = src.clone()
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = eng.nj_device(dd)   # (waits for the kernels: its results come back to the host)
        if rep:
            times.append(time.perf_counter() - t)
    return min(times), times, out


def reference_time(d, sample):
    import tree_ref as R
    n = d.shape[0]
    steps = n - 3 if sample is None else min(sample, n - 3)
    t = time.perf_counter()
    out = R.nj_np(d, steps=None if steps == n - 3 else steps)
    took = time.perf_counter() - t
    whole = sum(m * m for m in range(4, n + 1))
    part = sum(m * m for m in range(n - steps + 1, n + 1))
    return took * whole / part, steps, out


def search_time(eng, torch, n, launches):
    """Seconds of one search launch of n active slots, by difference."""
    from varkoder_amd import _capi
    idx = torch.arange(n, device=eng.device, dtype=torch.float64)   # (|i - j|: a valid matrix made on the device)
    dd = (idx[:, None] - idx[None, :]).abs()[None].contiguous()
    del idx
    ws = eng._workspace(eng.L.vk_tree_workspace_size, n, 1)
    status = torch.zeros(1, dtype=torch.int32, device=eng.device)

    def call(k):
        best = None
        for _ in range(4):
            torch.cuda.synchronize()
            t = time.perf_counter()
            st = eng.L.vk_tree_search_probe_device(eng.ctx, eng._ptr(dd), n, 1, k, eng._ptr(status), eng._ptr(ws), ws.numel())
            _capi.check(eng.ctx, st, "vk_tree_search_probe_device")
            torch.cuda.synchronize()
            took = time.perf_counter() - t
            best = took if best is None else min(best, took)
        return best
    few, many = call(4), call(4 + launches)
    assert int(status.cpu()[0]) == 0
    return (many - few) / launches


def trace(n):
    import torch
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    _, times, _ = device_time(eng, torch, matrix(n, 3)[None], 2)
    print(f"# three calls of one tree of {n} leaves (the first a warm-up); the last two took {[round(t * 1e3, 3) for t in times]} ms")
    eng.close()


def stats(path, wall_ms):
    total, rows = 0, []
    with open(path) as f:
        for row in csv.DictReader(f):
            if "vk_tr_" in row["Name"]:
                name = row["Name"].split("vk_tr_")[1].split("(")[0]
                rows.append((name, int(row["Calls"]), int(row["TotalDurationNs"])))
                total += int(row["TotalDurationNs"])
    for name, calls, ns in rows:
        print(f"vk_tr_{name:16s} {calls // 3:7d} launches a call  {ns / 3e6:9.3f} ms a call  {ns / calls / 1e3:8.2f} us each")
    per_call = total / 3e6
    share = 100 * (1 - per_call / wall_ms)
    print(f"kernels {per_call:.3f} ms of a call's {wall_ms:.3f} ms wall time: " +
          (f"{share:.1f} % of the call is spent between launches" if share > 0 else
           "nothing measurable is spent between launches (the profiler's own cost per launch is in the kernels' sum)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=40)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--skip-reference", action="store_true")
    ap.add_argument("--trace", type=int)
    ap.add_argument("--stats")
    ap.add_argument("--wall", type=float)
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats, a.wall)
    if a.trace:
        return trace(a.trace)
    import torch
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    print("# ImageEngine.nj_device (vk_tree_nj_device) against tests/tree_ref.py nj_np; device: best of "
          f"{a.reps} synchronised calls, matrix in HBM; reference: one run")
    for n, ntrees in ((256, 1), (1024, 1), (4096, 1), (256, 101)):
        d = np.stack([matrix(n, 3 + r) for r in range(ntrees)])
        best, times, out = device_time(eng, torch, d, a.reps)
        line = f"{ntrees:4d} x {n:5d} leaves  device {best * 1e3:10.2f} ms  ({2 * (n - 3) + 2} launches, {best / (2 * (n - 3) + 2) * 1e6:6.2f} us each)"
        if not a.skip_reference:
            ref, steps, rout = 0.0, 0, None
            timed = min(ntrees, 5)   # (of 101 trees five are timed and the sum scaled)
            for r in range(timed):
                t, steps, rout = reference_time(d[r], None if n < 4096 else a.sample)
                ref += t * ntrees / timed
                if steps == n - 3:   # (a whole run: the records must agree)
                    assert np.array_equal(out[1][r], rout[1]) and out[2][r].tobytes() == rout[2].tobytes(), (n, r)
            how = "whole runs, records equal" if steps == n - 3 else f"first {steps} steps, scaled"
            line += f"  NumPy {ref * 1e3:11.1f} ms ({how})  NumPy / device {ref / best:8.1f}"
        print(line, flush=True)
    print("# the search launch alone, all n slots active: bytes = 8 n (n - 1) / 2")
    for n in (1024, 4096, 8192, 16384):
        t = search_time(eng, torch, n, a.launches)
        b = 8.0 * n * (n - 1) / 2
        where = "Infinity Cache" if 8 * n * n <= 256e6 else "HBM"
        print(f"search {n:6d} leaves  {t * 1e6:9.2f} us  {b / 1e6:9.1f} MB  {b / t / 1e12:6.2f} TB/s  "
              f"{100 * b / t / HBM_PEAK:5.1f} % of 8.0 TB/s  {100 * b / t / HBM_COPY:5.1f} % of a copy's 6.29 TB/s  ({where})", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
