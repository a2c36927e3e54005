#!/usr/bin/env python3
"""Step C's files (vk_ladder_emit_device) on one cleaned sample: 1M reads x 150 bases by default (0.32 GB of text),
the default ladder (-m 500K -M 200M: the sample holds 150 Mbases, so its first step takes every read).  Prints one
JSON line: the emit call's time (best of --reps; the call waits for its kernels), the bytes it reads and writes,
the fraction of HBM peak that comes to, and beside it the copy back to the host and the host's gzip (level 1, one
thread) of the same text, so that a reader sees where an opt-in run's time goes.  Under `rocprofv3 --kernel-trace
--stats -- python tools/ladder_emit_time.py` the per-kernel times come from the trace.

The bytes counted: the text once per newline pass (two) and the records the steps take once for the plan's '\\r'
look-ups are not in it -- `moved_bytes` is the floor a perfect emit would move: the text once for the index, every
emitted byte read and written once.

--ab PARENT: the default path instead -- `image --from-clean` WITHOUT --write-splits over --ab-samples cleaned samples,
run in turn from this tree and from PARENT (a checkout of the parent commit with its library built: `git archive`
it into ab/parent, then `tools/build_rev.sh <rev> parent` and copy ab/parent.so to its varkoder_amd/libvkimg_hip.so),
--reps times each as a process of its own, alternated A B B A.  Prints one JSON line with each tree's wall times and
best; the parent's own spread is the yardstick for the difference.  Kernel names of the two come from a
`rocprofv3 --kernel-trace --stats` run of the same command on each tree.

usage: python tools/ladder_emit_time.py [--reads N] [--len L] [--reps R] [--peak-gb-s P]
       python tools/ladder_emit_time.py --ab PARENT [--ab-samples S] [--reads N] [--reps R]
"""
import argparse
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_reads(n, L, seed=1):
    """Text of n records `@rNNNNNNNN clean\\n<L>\\n+\\n<L>\\n`."""
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]
    seq[rng.random((n, L)) < 0.001] = ord("N")
    head = np.frombuffer(b"".join(b"@r%08d clean\n" % i for i in range(n)), dtype=np.uint8).reshape(n, -1)
    qual = (rng.integers(0, 41, (n, L)) + 33).astype(np.uint8)
    nl = np.full((n, 1), ord("\n"), dtype=np.uint8)
    plus = np.frombuffer(b"\n+\n", dtype=np.uint8)[None, :].repeat(n, axis=0)
    return np.concatenate([head, seq, plus, qual, nl], axis=1).ravel()


def run_ab(a):
    import shutil
    import subprocess
    import tempfile
    work = tempfile.mkdtemp(prefix="emit_ab_")
    try:
        clean = os.path.join(work, "clean")
        os.mkdir(clean)
        for i in range(a.ab_samples):   # (plain .fq: the files' inflate is not what is compared)
            make_reads(a.reads, a.len, seed=10 + i).tofile(os.path.join(clean, "s%02d.fq" % i))
        trees = {"this": ROOT, "parent": os.path.abspath(a.ab)}
        times = {name: [] for name in trees}
        order = ["this", "parent", "parent", "this"] * ((a.reps + 1) // 2)
        for n, name in enumerate(order):
            env = dict(os.environ, PYTHONPATH=trees[name])
            env.pop("VKIMG_LIB", None)
            out = os.path.join(work, "out%d" % n)
            t = time.perf_counter()
            subprocess.run([sys.executable, "-m", "varkoder_amd", "image", "--from-clean", clean, "-o", out, "-k", "7",
                            "-f", os.path.join(work, "stats%d.csv" % n)], cwd=trees[name], env=env, check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
            times[name].append(time.perf_counter() - t)
            pngs = sum(len(f) for _, _, f in os.walk(out))
            shutil.rmtree(out)
        print(json.dumps({"ab_samples": a.ab_samples, "reads": a.reads, "read_len": a.len, "pngs_last_run": pngs, "order": order,
                          "wall_s": times, "best_s": {k: min(v) for k, v in times.items()}}))
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--peak-gb-s", type=float, default=8000.0, help="HBM peak to state the fraction of")
    ap.add_argument("--ab", metavar="PARENT", help="time the default path of this tree against the tree at PARENT")
    ap.add_argument("--ab-samples", type=int, default=8)
    a = ap.parse_args()
    if a.ab:
        return run_ab(a)
    import torch
    from varkoder_amd.engine import ImageEngine
    from varkoder_amd.subsample import ladder_plan, plan_steps
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    text = make_reads(a.reads, a.len)
    dev, offs, lens = eng.upload([text])
    sync = torch.cuda.synchronize
    nsites, status = eng.read_index(dev, offs, lens)
    _, plans = ladder_plan(nsites, status, 500000, 200_000_000)
    steps = plan_steps(plans, nsites, 1)
    records = (eng.clean_lines(dev, offs, lens) + np.uint64(1)) // np.uint64(4)
    args = ([st[0] for st in steps], [st[3] for st in steps], [st[4] for st in steps], [st[5] for st in steps])
    # a first call finds the size (and is not timed); the timed ones write into a buffer of that size
    _, _, ol, _ = eng.ladder_emit(dev, offs, lens, *args, records=records)
    cap = int(((ol + np.uint64(15)) // np.uint64(16) * np.uint64(16)).sum())
    buf = torch.empty(cap + 64, dtype=torch.uint8, device=eng.device)
    best = []
    for _ in range(a.reps):
        sync()
        t = time.perf_counter()
        out, oo, ol, st = eng.ladder_emit(dev, offs, lens, *args, records=records, capacity=cap, out=buf)   # (waits for the kernels)
        best.append(time.perf_counter() - t)
    assert not st.any(), st
    emitted = int(ol.sum())
    sync()
    t = time.perf_counter()
    host = out[:cap].cpu().numpy()
    t_copy = time.perf_counter() - t
    t = time.perf_counter()
    packed = sum(len(gzip.compress(host[int(o):int(o) + int(n)].tobytes(), compresslevel=1)) for o, n in zip(oo, ol))
    t_gzip = time.perf_counter() - t
    emit_s = min(best)
    moved = int(lens[0]) + 2 * emitted
    print(json.dumps({
        "reads": a.reads, "read_len": a.len, "text_bytes": int(lens[0]), "steps": len(steps),
        "step_bp": [int(s[2]) for s in steps], "emitted_bytes": emitted, "emit_s_best": emit_s, "emit_s_all": best,
        "moved_bytes": moved, "moved_gb_s": moved / emit_s / 1e9, "fraction_of_peak": moved / emit_s / 1e9 / a.peak_gb_s,
        "peak_gb_s": a.peak_gb_s, "copy_back_s": t_copy, "copy_back_gb_s": emitted / t_copy / 1e9,
        "gzip1_s_one_thread": t_gzip, "gzip_bytes": packed}))
    eng.close()


if __name__ == "__main__":
    main()
