#!/usr/bin/env python3
"""`query --from-raw`, side measurement: the read-budget step of a folder of many small samples both ways, and the
whole command.

1. N synthetic files of R reads in HBM.  The mean length of each file's first 10,000 reads
   - by the host route that pipeline._budget took before vk_clean_heads_device existed, restated here: per file a
     device-to-host copy of at least 4 MiB of its head (4x more until it holds 40,001 newlines or the file ends) and
     rawinput.avg_read_length on the bytes;
   - by ImageEngine.clean_heads: one call, one synchronisation for the batch.
   Both give the same figures (asserted).  Each is timed --reps times after one untimed pass; the best and all are
   printed.
2. The same files written to a folder as plain `.fq`, then `python -m varkoder_amd query --from-raw` on it in a child
   process with a tiny seeded model: its wall time, start of the interpreter to exit.

Prints one JSON line.  usage: python tools/query_raw_time.py [--files N] [--reads R] [--reps K] [--no-e2e] [--tmp DIR]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_route(dev, offs, lens):
    """The means as the parent of the heads kernel got them (pipeline._budget, max_bp given)."""
    from varkoder_amd.rawinput import avg_read_length
    avgs = []
    for j in range(len(offs)):
        o, n, take = int(offs[j]), int(lens[j]), 4 << 20
        while True:
            head = dev[o:o + min(n, take)].cpu().numpy().tobytes()
            if take >= n or head.count(b"\n") >= 4 * 10000 + 1:
                break
            take *= 4
        avgs.append(round(avg_read_length(head)))
    return avgs


def kernel_route(eng, dev, offs, lens):
    totals, counted = eng.clean_heads(dev, offs, lens, 10000)
    return [round(int(t) / int(n)) if n else 0 for t, n in zip(totals, counted)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--tmp", default=None, help="where the folder of files is made (default: the system's temporary folder)")
    a = ap.parse_args()
    import torch
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    dev, offs, lens = eng.synth(0, a.files, a.reads, a.len, dist=1)
    torch.cuda.synchronize()
    out = {"files": a.files, "reads_per_file": a.reads, "read_length": a.len, "text_bytes": int(lens.sum())}
    want = host_route(dev, offs, lens)          # (untimed passes: the first launch loads the code object)
    assert kernel_route(eng, dev, offs, lens) == want
    out["avg_length_first_file"] = want[0]
    for name, fn in (("host_route", lambda: host_route(dev, offs, lens)), ("clean_heads", lambda: kernel_route(eng, dev, offs, lens))):
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = fn()
            times.append(time.perf_counter() - t)   # (both routes end in a copy to the host: the device is done)
            assert got == want
        out[name + "_s_best"], out[name + "_s_all"] = min(times), times
        print(name, times, file=sys.stderr, flush=True)
    if not a.no_e2e:
        tmp = tempfile.mkdtemp(prefix="query_raw_time_", dir=a.tmp)
        try:
            raw = os.path.join(tmp, "raw")
            os.mkdir(raw)

            def write(j, blob):
                with open(os.path.join(raw, "s%05d.fq" % j), "wb") as f:
                    f.write(blob)
            with ThreadPoolExecutor(8) as pool:
                step = 50
                for j0 in range(0, a.files, step):
                    lo, hi = int(offs[j0]), int(offs[min(j0 + step, a.files) - 1] + lens[min(j0 + step, a.files) - 1])
                    host = dev[lo:hi].cpu().numpy()
                    for j in range(j0, min(j0 + step, a.files)):
                        pool.submit(write, j, host[int(offs[j]) - lo:int(offs[j]) - lo + int(lens[j])].tobytes())
            del dev
            eng.close()
            print("files written", file=sys.stderr, flush=True)
            torch.manual_seed(3)
            model = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(6), torch.nn.Flatten(1), torch.nn.Linear(3 * 36, 4))
            torch.jit.script(model).save(os.path.join(tmp, "m.pt"))
            with open(os.path.join(tmp, "vocab.txt"), "w") as f:
                f.write("a\nb\nc\nd\n")
            env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
            t = time.perf_counter()
            p = subprocess.run([sys.executable, "-m", "varkoder_amd", "query", raw, os.path.join(tmp, "out"), "-l",
                                os.path.join(tmp, "m.pt"), "--vocab", os.path.join(tmp, "vocab.txt"), "--from-raw", "-n", "8"],
                               capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
            out["query_from_raw_wall_s"] = time.perf_counter() - t
            if p.returncode != 0:
                out["query_from_raw_error"] = p.stderr[-1500:]
            else:
                with open(os.path.join(tmp, "out", "predictions.csv")) as f:
                    out["prediction_rows"] = sum(1 for _ in f) - 1
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out), flush=True)
    return 1 if "query_from_raw_error" in out else 0


if __name__ == "__main__":
    sys.exit(main())
