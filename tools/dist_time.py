#!/usr/bin/env python3
"""`compare`'s call (vk_dist_device, ImageEngine.neighbours) beside torch's route on the same device in one process:
--images synthetic 91 x 91 images (k = 7 varKodes' size) against themselves, the --neighbours nearest others of each.
The images come in families of --family (a base image and noisy copies, as the bp steps of a sample resemble each
other, some copies exact), so near-ties exist.  Torch's route is what a user would write: an fp32 `Q @ Q.T`, the norms
added, the diagonal masked, `torch.topk`.  Synchronised wall time of both, alternating, best of --reps after a warm-up
of each; the multiply-adds (images^2 x pixels) per second of both; and how many of the torch route's rows of
neighbours differ from the exact ones (its sums pass 2^24, so near-ties come out in an arbitrary order).  Under
`rocprofv3 --kernel-trace --stats -- python tools/dist_time.py --reps 1` the per-kernel times come from the trace.

usage: python tools/dist_time.py [--images N] [--side S] [--neighbours K] [--family F] [--reps R]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20000)
    ap.add_argument("--side", type=int, default=91)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--family", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    n, p, k = a.images, a.side * a.side, a.neighbours
    g = torch.Generator(device=eng.device).manual_seed(1)
    nfam = (n + a.family - 1) // a.family
    base = torch.randint(0, 256, (nfam, 1, p), generator=g, device=eng.device, dtype=torch.int16)
    # member m of a family: noise of amplitude 0, 0 (two exact copies), 1, 2, 4, ..
    amp = torch.tensor([0, 0] + [1 << i for i in range(a.family - 2)], device=eng.device, dtype=torch.int16).clamp(max=64)
    noise = torch.randint(-64, 65, (nfam, a.family, p), generator=g, device=eng.device, dtype=torch.int16)
    x = (base + noise * amp.view(1, -1, 1) // 64).clamp(0, 255).to(torch.uint8).reshape(-1, p)[:n].contiguous()
    del base, noise
    own = np.arange(n, dtype=np.uint32)
    sync = torch.cuda.synchronize

    def exact():
        return eng.neighbours(x, x, n=k, qgroup=own, rgroup=own)

    def torch_route():
        f = x.float()
        sq = (f * f).sum(1)
        d = sq[:, None] + sq[None, :] - 2.0 * (f @ f.T)
        d.fill_diagonal_(float("inf"))
        v, i = torch.topk(d, k, dim=1, largest=False)
        return i.cpu().numpy(), v.cpu().numpy()

    times = {"exact": [], "torch": []}
    got = {}
    for rep in range(a.reps + 1):   # (the first round warms both up)
        for name, call in (("exact", exact), ("torch", torch_route)):
            sync()
            t = time.perf_counter()
            got[name] = call()   # (waits for the kernels: its results come back to the host)
            if rep:
                times[name].append(time.perf_counter() - t)
    t_exact, t_torch = min(times["exact"]), min(times["torch"])
    idx = got["exact"][0].astype(np.int64)
    differ = int((idx != got["torch"][0]).any(axis=1).sum())
    unordered = int((np.sort(idx, axis=1) != np.sort(got["torch"][0], axis=1)).any(axis=1).sum())
    macs = n * n * p
    print(f"# {n} images of {a.side} x {a.side} against themselves, {k} neighbours, families of {a.family}; best of {a.reps}, "
          f"all of {a.reps}: exact {[round(t * 1e3, 1) for t in times['exact']]} torch {[round(t * 1e3, 1) for t in times['torch']]} ms")
    print(f"ImageEngine.neighbours (i8 matrix cores, exact)  {t_exact * 1e3:9.2f} ms  {macs / t_exact / 1e12:8.2f} T multiply-adds/s")
    print(f"torch: fp32 Q @ Q.T + norms + topk               {t_torch * 1e3:9.2f} ms  {macs / t_torch / 1e12:8.2f} T multiply-adds/s")
    print(f"exact / torch                                    {t_exact / t_torch:9.3f}")
    print(f"rows of the torch route that differ from the exact ones: {differ} of {n} ({unordered} also as sets)")
    eng.close()


if __name__ == "__main__":
    main()
