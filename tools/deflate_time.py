#!/usr/bin/env python3
"""The BGZF compressor (vk_deflate_device) on one cleaned sample: 1M reads x 150 bases from the shaped generator
(synth dist 2: reads as step B leaves them), or the text of FILE (.gz is read through gzip).  Prints one JSON line:
the call's time (best of --reps, synchronised; workspace and output allocated ahead) as GB/s of text, the host's
gzip.compress(level 1) of the same text on 1 thread and on 16 (the text cut in 16, a thread each: zlib releases the GIL),
the size each of them writes, and the copy back to the host of the text against that of the compressed bytes.

--e2e: `image --from-clean -i INT --write-splits` over --samples cleaned samples with and without --gpu-gzip, each run a
process of its own under its own time limit (--limit seconds), alternated A B B A ..., exactly --reps times each; a run
that fails or runs out of time ends the series, with the end of its stderr on this program's.  Prints one JSON line with
each side's wall times and best; the side without the flag is the yardstick.

The first form is one GPU step and has no limit of its own: run it under one, and chain steps with &&, e.g.
    timeout -k 10 200 python tools/deflate_time.py && timeout -k 10 900 python tools/deflate_time.py --e2e

usage: python tools/deflate_time.py [FILE] [--reads N] [--len L] [--reps R]
       python tools/deflate_time.py --e2e [--samples S] [--reads N] [--reps R]
"""
import argparse
import ctypes as C
import gzip
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_e2e(a):
    import shutil
    import subprocess
    import tempfile
    import torch
    from varkoder_amd.engine import ImageEngine
    work = tempfile.mkdtemp(prefix="deflate_e2e_")
    try:
        clean = os.path.join(work, "int", "clean_reads")
        os.makedirs(clean)
        eng = ImageEngine(k=7, mapping="cgr", device=0)
        for i in range(a.samples):   # (plain .fq: the files' inflate is not what is compared)
            dev, offs, lens = eng.synth(10 + i, 1, a.reads, a.len, dist=2)
            dev[:int(lens[0])].cpu().numpy().tofile(os.path.join(clean, "s%02d.fq" % i))
        eng.close()
        del dev
        torch.cuda.empty_cache()
        times = {"host_gzip": [], "gpu_gzip": []}
        order = [name for i in range(a.reps) for name in (("gpu_gzip", "host_gzip") if i % 2 == 0 else ("host_gzip", "gpu_gzip"))]
        sizes = {}
        for n, name in enumerate(order):
            out = os.path.join(work, "out%d" % n)
            argv = [sys.executable, "-m", "varkoder_amd", "image", "--from-clean", os.path.join(work, "int"), "-i",
                    os.path.join(work, "int"), "--write-splits", "-x", "-o", out, "-k", "7", "-n", "16",
                    "-f", os.path.join(work, "stats%d.csv" % n)] + (["--gpu-gzip"] if name == "gpu_gzip" else [])
            t = time.perf_counter()
            try:   # (a failure or the limit raises: nothing more is started)
                subprocess.run(argv, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), check=True, stdout=subprocess.DEVNULL,
                               stderr=subprocess.PIPE, timeout=a.limit)
            except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
                sys.stderr.write("run %d (%s) ended the series: %r\n%s\n" % (n, name, e, (e.stderr or b"")[-2000:].decode("replace")))
                raise
            times[name].append(time.perf_counter() - t)
            d = os.path.join(work, "int", "split_fastqs")
            sizes[name] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
            shutil.rmtree(out)
        print(json.dumps({"e2e_samples": a.samples, "reads": a.reads, "read_len": a.len, "order": order, "wall_s": times,
                          "best_s": {k: min(v) for k, v in times.items()}, "split_fastqs_bytes": sizes}))
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file", nargs="?")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--limit", type=int, default=300, help="--e2e: seconds a run may take")
    a = ap.parse_args()
    if a.e2e:
        return run_e2e(a)
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine, _u64
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    if a.file:
        with (gzip.open if a.file.endswith(".gz") else open)(a.file, "rb") as f:
            dev, offs, lens = eng.upload([f.read()])
    else:
        dev, offs, lens = eng.synth(1, 1, a.reads, a.len, dist=2)
    n = int(lens[0])
    sync = torch.cuda.synchronize
    bound, wsb = C.c_uint64(), C.c_uint64()
    eng.L.vk_deflate_bound(_u64(lens), 1, C.byref(bound))
    eng.L.vk_deflate_workspace_size(_u64(lens), 1, C.byref(wsb))
    out = torch.empty(bound.value, dtype=torch.uint8, device=eng.device)
    ws = torch.empty(max(wsb.value, 256), dtype=torch.uint8, device=eng.device)
    oo, ol = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    runs = []
    for _ in range(a.reps + 1):   # (the first one warms up and is not kept)
        sync()
        t = time.perf_counter()
        _capi.check(eng.ctx, eng.L.vk_deflate_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), 1, eng._ptr(out), bound.value,
                                                     eng._ptr(ws), ws.numel(), _u64(oo), _u64(ol)), "vk_deflate_device")
        runs.append(time.perf_counter() - t)   # (the call waits for its kernels)
    runs = runs[1:]
    packed = int(ol[0])
    copies = {}
    for name, t_dev in (("text", dev[:n]), ("compressed", out[:packed])):
        sync()
        t = time.perf_counter()
        host = t_dev.cpu().numpy()
        copies[name] = time.perf_counter() - t
        if name == "text":
            text = host.tobytes()
    assert gzip.decompress(host.tobytes()) == text, "the file does not inflate to the text"
    t = time.perf_counter()
    g1 = len(gzip.compress(text, compresslevel=1))
    t1 = time.perf_counter() - t
    cut = [text[i * n // 16:(i + 1) * n // 16] for i in range(16)]
    with ThreadPoolExecutor(16) as pool:
        t = time.perf_counter()
        g16 = sum(len(b) for b in pool.map(lambda b: gzip.compress(b, compresslevel=1), cut))
        t16 = time.perf_counter() - t
    best = min(runs)
    print(json.dumps({
        "text_bytes": n, "deflate_s_best": best, "deflate_s_all": runs, "deflate_gb_s_of_text": n / best / 1e9,
        "deflate_bytes": packed, "gzip1_bytes": g1, "size_vs_gzip1": packed / g1, "gzip1_s_one_thread": t1,
        "gzip1_gb_s_one_thread": n / t1 / 1e9, "gzip1_s_16_threads": t16, "gzip1_gb_s_16_threads": n / t16 / 1e9,
        "gzip1_bytes_16_pieces": g16, "copy_back_s_text": copies["text"], "copy_back_s_compressed": copies["compressed"]}))
    eng.close()


if __name__ == "__main__":
    main()
