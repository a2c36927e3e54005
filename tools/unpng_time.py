#!/usr/bin/env python3
"""--gpu-png-read (pngread.read_images, vk_unpng_device) beside the route both commands take without it (PIL decode of
every file, np.stack, one copy to HBM), in one process, on folders of PIL-written files (optimize=True, as `image`
writes them):
    side128     --n128 files of 128 x 128: 7-level Poisson images (png_cases.levels7: what a window's image looks like)
                and the three golden cgr images of tests/golden/*.png (real varKodes), alternating
    side512     --n512 files of 512 x 512: 7-level images and the golden images tiled 4 x 4, alternating
Per folder, --warmup warm-ups and --reps runs each, median / min / max of synchronised wall time:
    read        the files' bytes alone (both routes pay it), on 1 thread and on 16
    pil         np.array(Image.open(p)) of every file, np.stack, .to(device): on 1 thread (what `train` and `query
                --images` do today) and with the decodes on 16 threads (what they could do on the host)
    gpu         read_images(engine, paths) without a pool, and with a pool of 16 reading the files
    unpng       ImageEngine.unpng alone on the streams laid out beforehand (copy to HBM, two kernels, statuses back)
The files are read once before anything is timed: they come from the page cache in every run.  One JSON line per row
and a table.

One GPU; run it under a time limit:
    timeout -k 10 600 python tools/unpng_time.py
"""
import argparse
import glob
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    return {"ms": round(float(np.median(ms)), 2), "min_max": [round(min(ms), 2), round(max(ms), 2)]}


def timed(fn, warmup, reps, sync):
    ms = []
    for r in range(warmup + reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if r >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def write_folder(d, side, n, seed):
    import png_cases as P
    from PIL import Image
    rng = np.random.default_rng(seed)
    golden = [np.array(Image.open(p)) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*+cgr+k7.png")))]
    assert golden and all(g.shape == (128, 128) for g in golden)
    paths = []
    for i in range(n):
        if i % 2 == 0:
            arr = P.levels7(rng, side)
        else:
            arr = np.tile(golden[(i // 2) % len(golden)], (side // 128, side // 128))
        p = os.path.join(d, f"s{i:06d}@00010000K+cgr+k{7 if side == 128 else 9}.png")
        Image.fromarray(arr).save(p, format="PNG", optimize=True)
        paths.append(p)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n128", type=int, default=4000)
    ap.add_argument("--n512", type=int, default=400)
    ap.add_argument("--seed", type=int, default=20260102)
    a = ap.parse_args()
    import torch
    from PIL import Image
    from varkoder_amd import pngread as R
    from varkoder_amd.engine import ImageEngine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    print(json.dumps({"warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)}), flush=True)
    sync = torch.cuda.synchronize
    rows = []
    for name, side, n in (("side128", 128, a.n128), ("side512", 512, a.n512)):
        with tempfile.TemporaryDirectory() as d:
            paths = write_folder(d, side, n, a.seed + side)
            eng = ImageEngine(k=7 if side == 128 else 9, mapping="cgr", device=0)
            datas = [R.read_file(p) for p in paths]
            parts = [R.png_parts(x) for x in datas]
            assert all(R.eligible(p) for p in parts)
            filters = np.zeros(5, dtype=np.int64)
            for x, p in list(zip(datas, parts))[:50]:
                raw = zlib.decompress(b"".join(x[s:e] for s, e in p.spans))
                filters += np.bincount(np.frombuffer(raw, dtype=np.uint8).reshape(side, side + 1)[:, 0], minlength=5)[:5]
            streams = R.pack_streams(datas, parts, side)

            def pil1():
                return torch.from_numpy(np.stack([np.array(Image.open(p)) for p in paths])).to(eng.device)

            def pil16():
                with ThreadPoolExecutor(16) as pool:
                    return torch.from_numpy(np.stack(list(pool.map(R.pil_array, paths)))).to(eng.device)

            def read16():
                with ThreadPoolExecutor(16) as pool:
                    return list(pool.map(R.read_file, paths))

            def gpu16():
                with ThreadPoolExecutor(16) as pool:
                    return R.read_images(eng, paths, pool=pool)
            want = pil1()
            assert torch.equal(R.read_images(eng, paths), want) and torch.equal(pil16(), want)
            row = {"set": name, "files": n, "file_bytes": sum(map(len, datas)), "filter_rows_in_50": filters.tolist(),
                   "read1": timed(lambda: [R.read_file(p) for p in paths], a.warmup, a.reps, sync),
                   "read16": timed(read16, a.warmup, a.reps, sync),
                   "pil1": timed(pil1, a.warmup, a.reps, sync),
                   "pil16": timed(pil16, a.warmup, a.reps, sync),
                   "gpu1": timed(lambda: R.read_images(eng, paths), a.warmup, a.reps, sync),
                   "gpu16": timed(gpu16, a.warmup, a.reps, sync),
                   "unpng": timed(lambda: eng.unpng(streams, side), a.warmup, a.reps, sync)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            eng.close()
    print(f"{'set':8} {'files':>6} {'read1':>8} {'read16':>8} {'pil1':>9} {'pil16':>9} {'gpu1':>8} {'gpu16':>8} {'unpng':>8}   (ms, medians)")
    for r in rows:
        print(f"{r['set']:8} {r['files']:6d} {r['read1']['ms']:8.1f} {r['read16']['ms']:8.1f} {r['pil1']['ms']:9.1f} {r['pil16']['ms']:9.1f} "
              f"{r['gpu1']['ms']:8.1f} {r['gpu16']['ms']:8.1f} {r['unpng']['ms']:8.1f}")


if __name__ == "__main__":
    main()
