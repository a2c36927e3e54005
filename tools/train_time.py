"""Time one epoch's batch building for `train`, two ways: the batch kernel (vk_train_batch_device) and the same rule
composed from torch ops on the GPU (index, query.preprocess, logit / sigmoid, lerp).

    python tools/train_time.py [--images 4096] [--side 128] [--out 224] [--batch 64] [--repeats 7]

The set (k = 7 sized images by default), MixUp plus lighting parameters and the visiting order are drawn once from a
seed; both ways get the same ones, including the per-step copy of the parameters to the device.  An epoch is timed with
a host clock around work that ends in a device synchronise; the two ways alternate, after one warm-up epoch each.
Prints one JSON line: seconds per epoch (median and best) of each, and torch / kernel."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--out", type=int, default=224)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import torch
    from varkoder_amd import query as Q
    from varkoder_amd import train as T
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    g = torch.Generator().manual_seed(11)
    images = torch.randint(0, 256, (a.images, a.side, a.side), generator=g, dtype=torch.uint8).to(eng.device)
    steps = a.images // a.batch
    order = torch.randperm(a.images, generator=g).numpy().astype(np.uint32)
    params = [T.draw_batch_params(g, a.batch, a.out, T.MODE_MIXUP, 0.75, 0.25) for _ in range(steps)]
    out = torch.empty((a.batch, 3, a.out, a.out), dtype=torch.float32, device=eng.device)

    def kernel_step(s):
        p = params[s]
        return T.train_batch(eng, images, order[s * a.batch:(s + 1) * a.batch], p["partner"], p["lam"], p["bshift"], p["cscale"],
                             p["rect"], T.MODE_MIXUP, a.out, out=out)

    def torch_step(s):
        p = params[s]
        dev = eng.device
        idx = torch.from_numpy(order[s * a.batch:(s + 1) * a.batch].astype(np.int64)).to(dev)
        partner = torch.from_numpy(p["partner"].astype(np.int64)).to(dev)
        lam, b, c = (torch.from_numpy(p[k]).to(dev)[:, None, None, None] for k in ("lam", "bshift", "cscale"))
        s0 = Q.preprocess(eng, images[idx].contiguous(), out_size=a.out, mean=T.MEAN, std=T.STD)
        x = (s0 * T.STD + T.MEAN).clamp(1e-7, 1.0 - 1e-7)
        lit = (torch.sigmoid((torch.logit(x) + b) * c) - T.MEAN) / T.STD
        s1 = torch.where((b != 0) | (c != 1), lit, s0)
        return torch.lerp(s1[partner], s1, lam)   # lam * s + (1 - lam) * s_partner

    def epoch(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(steps):
            step(s)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    diff = float((kernel_step(0) - torch_step(0)).abs().max())
    epoch(kernel_step), epoch(torch_step)
    tk, tt = [], []
    for _ in range(a.repeats):
        tk.append(epoch(kernel_step))
        tt.append(epoch(torch_step))
    eng.close()
    mk, mt = statistics.median(tk), statistics.median(tt)
    print(json.dumps({"images": a.images, "side": a.side, "out": a.out, "batch": a.batch, "steps": steps, "repeats": a.repeats,
                      "kernel_epoch_s_median": mk, "kernel_epoch_s_best": min(tk), "torch_epoch_s_median": mt,
                      "torch_epoch_s_best": min(tt), "torch_over_kernel": mt / mk, "max_abs_diff_first_batch": diff,
                      "output_bytes_per_epoch": steps * a.batch * 3 * a.out * a.out * 4}))


if __name__ == "__main__":
    main()
