#!/usr/bin/env python3
"""The PNG encoder (ImageEngine.png, vk_png_device) beside the host's (image.write_png into BytesIO: PIL, optimize=True)
in one process, on three sets of images made on the device:
    dense7      9,000 images of k = 7 (cgr, 128 x 128) of read samples: histograms of Poisson counts with mean 40, which
                rank-binning spreads over all 256 levels
    dense9      1,000 images of k = 9 (cgr, 512 x 512), the same way
    windows     100,000 images of k = 7 of the windows of an assembly at (N, S) = (10000, 2500): Poisson counts with
                mean 10000 / 4^7 = 0.61, seven or eight grey levels
The histograms are drawn with torch.poisson on the device and imaged by ImageEngine.images: what a count of uniform
synthetic reads / of a uniform synthetic assembly gives, without the minutes that counting them would take here.
engine.png: synchronised wall time, --warmup warm-ups and --reps runs, median / min / max.  write_png: the same images
(the first --host-sample of a set; 0 = all) into BytesIO on 1 thread and on 16, per image and scaled to the set.
Both outputs' total bytes.  One JSON line per row and a table.

--e2e: `image --from-fasta --windows --window-length 10000 --window-step 2500 -n 16` on a synthetic assembly of
--e2e-mbases Mbase (uniform ACGT, 60-column lines, one record; 250 gives the 100,000 windows above), with and without
--gpu-png, alternated, a process per run, three each: wall seconds of every run.

One GPU; run it under a time limit:
    timeout -k 10 900 python tools/png_time.py [--e2e]
"""
import argparse
import io
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = (("dense7", 7, 9000, 40.0), ("dense9", 9, 1000, 40.0), ("windows", 7, 100000, 10000 / 4 ** 7))
TEXT = (["genus:Aus", "species:Aus bus"], 0.01, 0.01, "cgr")


def stats(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_max": [round(min(ms), 3), round(max(ms), 3)]}


def images_of(torch, eng, n, mean, seed):
    """n images of the engine's k from Poisson histograms, made in slices of at most 2 GiB of histogram"""
    gen = torch.Generator(device=eng.device).manual_seed(seed)
    img = torch.empty((n, eng.side, eng.side), dtype=torch.uint8, device=eng.device)
    step = max(1, (2 << 30) // (4 * eng.ncode))
    for i0 in range(0, n, step):
        m = min(step, n - i0)
        rate = torch.full((m, eng.ncode), mean, dtype=torch.float32, device=eng.device)
        eng.images(torch.poisson(rate, generator=gen).to(torch.int32), img=img[i0:i0 + m])
    return img


def host_encode(arr):
    from PIL import Image
    from varkoder_amd.image import _text_chunks
    buf = io.BytesIO()   # (write_png's own call; a BytesIO has no name to take the format from)
    Image.fromarray(arr).save(buf, format="PNG", optimize=True, pnginfo=_text_chunks(*TEXT))
    return buf.tell()


def e2e(mbases, seed):
    rng = np.random.default_rng(seed)
    with tempfile.TemporaryDirectory() as d:
        os.mkdir(os.path.join(d, "fa"))
        n = int(mbases * 1e6) // 60 * 60
        lines = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n, dtype=np.uint8)].reshape(-1, 60)
        text = np.concatenate([lines, np.full((len(lines), 1), 10, dtype=np.uint8)], axis=1)
        with open(os.path.join(d, "fa", "asm.fa"), "wb") as f:
            f.write(b">chr1\n" + text.tobytes())
        del lines, text
        for rep in range(3):
            for flag in ((), ("--gpu-png",)):
                out = os.path.join(d, f"out{rep}{len(flag)}")
                cmd = [sys.executable, "-m", "varkoder_amd", "image", os.path.join(d, "fa"), "--from-fasta", "--windows",
                       "--window-length", "10000", "--window-step", "2500", "-k", "7", "-n", "16", "-o", out,
                       "-f", os.path.join(d, "stats.csv"), *flag]
                t0 = time.perf_counter()
                r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
                dt = time.perf_counter() - t0
                if r.returncode:
                    raise SystemExit(f"run failed ({r.returncode}): {r.stderr[-1500:]}")
                files = sum(len(fs) for _, _, fs in os.walk(out))
                size = sum(os.path.getsize(os.path.join(p, f)) for p, _, fs in os.walk(out) for f in fs)
                print(json.dumps({"e2e": "gpu-png" if flag else "default", "rep": rep, "mbases": mbases, "seconds": round(dt, 2),
                                  "files": files, "bytes": size}), flush=True)
                subprocess.run(["rm", "-rf", out])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20260101)
    ap.add_argument("--host-sample", type=int, default=0, help="images of a set that write_png is timed on (0: all)")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of every set's images (a quick look)")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-mbases", type=float, default=250.0)
    a = ap.parse_args()
    import torch
    from varkoder_amd.engine import ImageEngine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    if a.e2e:
        return e2e(a.e2e_mbases, a.seed)
    print(json.dumps({"warmup": a.warmup, "reps": a.reps, "host_sample": a.host_sample, "device": torch.cuda.get_device_name(0)}),
          flush=True)
    rows = []
    for name, k, n, mean in SETS:
        n = max(1, int(n * a.scale))
        eng = ImageEngine(k=k, mapping="cgr", device=0)
        img = images_of(torch, eng, n, mean, a.seed + k)
        levels = int(torch.unique(img[:64]).numel())
        ms, total = [], 0
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            chunks = eng.png(img)
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            total = sum(map(len, chunks))
        m = n if a.host_sample == 0 else min(n, a.host_sample)
        host = img[:m].cpu().numpy()
        row = {"set": name, "k": k, "images": n, "levels_in_64": levels, "gpu": stats(ms), "gpu_us_per_image": round(np.median(ms) * 1e3 / n, 2),
               "gpu_idat_bytes": total, "host_images": m}
        for threads in (1, 16):
            t0 = time.perf_counter()
            with ThreadPoolExecutor(threads) as pool:
                sizes = list(pool.map(host_encode, host))
            dt = time.perf_counter() - t0
            row[f"host{threads}_ms_per_image"] = round(dt * 1e3 / m, 3)
            row[f"host{threads}_s_for_the_set"] = round(dt * n / m, 2)
        row["host_file_bytes_per_image"] = round(sum(sizes) / m, 1)
        row["gpu_idat_bytes_per_image"] = round(total / n, 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del img, host
        eng.close()
    print(f"{'set':10} {'images':>8} {'png ms':>10} {'us/img':>8} {'host1 s':>9} {'host16 s':>9} {'B/img gpu':>10} {'B/img PIL':>10}")
    for r in rows:
        print(f"{r['set']:10} {r['images']:8d} {r['gpu']['ms']:10.1f} {r['gpu_us_per_image']:8.2f} {r['host1_s_for_the_set']:9.2f} "
              f"{r['host16_s_for_the_set']:9.2f} {r['gpu_idat_bytes_per_image']:10.1f} {r['host_file_bytes_per_image']:10.1f}")


if __name__ == "__main__":
    main()
