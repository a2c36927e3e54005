#!/usr/bin/env python3
"""The k-mer spectrum (vk_spectrum_device, ImageEngine.spectrum: `--kmer-spectrum`) on 2 x --pairs synthetic reads of
--len bases with 0.5 % substitutions, both strands, as one cleaned FASTQ text in HBM:

  shallow   reads from a random genome large enough for 0.3x: nearly every window inserts a new key
  deep      reads from a genome small enough for 30x: nearly every window re-hits a key
  repeats   the deep reads with a quarter replaced, half by poly-A and half by (ACGT)n: whole waves on one or two slots

each at K = 21 and 31 and every = 1 and 16.  Prints per run the engine call's time (best of --reps, device-synchronised:
the tables' allocation, the read index, the init, count and histogram kernels and the rows' copy), the windows per
second, the tables' bytes and load, beside vk_clean_device's time on the same reads as pairs in the same run and the two
figures of profiles/ab/screen_time.txt that bracket the count: the insert rate of vk_sc_build_kernel<true> and the window
rate of vk_sc_match_kernel.  Then, at K = 21 and every = 1, each workload with VKIMG_SPECTRUM_MERGE = 0, 1, 2 (how the
count kernel merges equal keys of a wave instruction).  Under `rocprofv3 --kernel-trace --stats -- python
tools/spectrum_time.py --reps 1` the per-kernel times come from the trace.

usage: python tools/spectrum_time.py [--pairs N] [--len L] [--reps R] [--no-merge-sweep]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUILD_KEYS_PER_S = 16e6 / 9.9e-3      # vk_sc_build_kernel<true>, profiles/ab/screen_time.txt
MATCH_WINDOWS_PER_S = 190e6 / 4.7e-3  # vk_sc_match_kernel, the same record
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def reads_of(rng, genome_len, n, L, error=0.005, chunk=250_000):
    """n reads (uint8 letters, [n, L]) from a random genome, either strand, substitutions at `error`."""
    g = rng.integers(0, 4, genome_len, dtype=np.uint8)
    out = np.empty((n, L), dtype=np.uint8)
    comp = np.array([3, 2, 1, 0], dtype=np.uint8)
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        at = rng.integers(0, genome_len - L + 1, m)
        r = g[at[:, None] + np.arange(L)[None, :]]
        flip = rng.random(m) < 0.5
        r[flip] = comp[r[flip][:, ::-1]]
        err = rng.random(r.shape) < error
        r[err] = (r[err] + rng.integers(1, 4, int(err.sum()), dtype=np.uint8)) & 3
        out[a:a + m] = ACGT[r]
    return out


def fastq_of(reads, tag=b"p"):
    """Fixed-size records `@pNNNNNNNN\\n<L>\\n+\\n<L>\\n` as one uint8 array."""
    n, L = reads.shape
    rec = np.empty((n, 11 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1] = tag[0]
    idx = np.arange(n)
    for d in range(8):
        rec[:, 9 - d] = ord("0") + (idx // 10 ** d) % 10
    rec[:, 10] = ord("\n")
    rec[:, 11:11 + L] = reads
    rec[:, 11 + L:14 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 14 + L:14 + 2 * L] = ord("I")
    rec[:, 14 + 2 * L] = ord("\n")
    return rec.ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-merge-sweep", action="store_true")
    a = ap.parse_args()
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine
    sync = torch.cuda.synchronize
    n, L = 2 * a.pairs, a.len
    rng = np.random.default_rng(7)
    bases = n * L
    work = {"shallow": reads_of(rng, int(bases / 0.3), n, L), "deep": reads_of(rng, bases // 30, n, L)}
    rep = work["deep"].copy()
    rep[0::8] = ord("A")
    rep[4::8] = np.resize(ACGT, L)
    work["repeats"] = rep
    print(f"# {n} reads x {L} bp ({a.pairs} pairs), 0.5 % substitutions, best of {a.reps}; times in ms")
    print(f"# parent-commit figures: vk_sc_build_kernel<true> {BUILD_KEYS_PER_S / 1e9:.2f} G keys/s inserted, "
          f"vk_sc_match_kernel {MATCH_WINDOWS_PER_S / 1e9:.1f} G windows/s formed and probed")

    def engine(merge=None):
        old = os.environ.pop("VKIMG_SPECTRUM_MERGE", None)
        if merge is not None:
            os.environ["VKIMG_SPECTRUM_MERGE"] = str(merge)
        try:
            return ImageEngine(k=7, mapping="cgr", device=0)
        finally:
            os.environ.pop("VKIMG_SPECTRUM_MERGE", None)
            if old is not None:
                os.environ["VKIMG_SPECTRUM_MERGE"] = old

    def timed(eng, dev, offs, lens, k, every):
        best = []
        for _ in range(a.reps):
            sync()
            t = time.perf_counter()
            rows, status = eng.spectrum(dev, offs, lens, k=k, every=every, records=[n])   # (waits for the kernels)
            best.append(time.perf_counter() - t)
        assert not status.any(), status
        return min(best), rows[0]

    eng = engine()
    sweep = {}
    for name, reads in work.items():
        # vk_clean_device on the same reads, as pairs
        pdev, poffs, plens = eng.upload([fastq_of(reads[:a.pairs]), fastq_of(reads[a.pairs:])])
        recs = eng.clean_lines(pdev, poffs, plens) // 4
        clean = []
        for _ in range(a.reps):
            sync()
            t = time.perf_counter()
            eng.clean(pdev, poffs, plens, recs, [_capi.VK_CL_ROLE_R1, _capi.VK_CL_ROLE_R2], [0, 0], 1)   # (waits for the kernels)
            clean.append(time.perf_counter() - t)
        del pdev
        dev, offs, lens = eng.upload([fastq_of(reads)])
        print(f"{name}: text {int(lens[0])} bytes, vk_clean_device {min(clean) * 1e3:.2f}")
        for k in (21, 31):
            for every in (1, 16):
                s, row = timed(eng, dev, offs, lens, k, every)
                slots = eng.spectrum_slots(int(lens[0]), every)
                wps = int(row[2]) / s
                print(f"  K {k} every {every:2d}: spectrum {s * 1e3:8.2f}  windows {int(row[2])} taken {int(row[3])} distinct {int(row[4])}  "
                      f"{wps / 1e9:6.2f} G windows/s ({wps / BUILD_KEYS_PER_S:5.2f} x build, {wps / MATCH_WINDOWS_PER_S:5.3f} x match)  "
                      f"tables {slots * 12 / 2**20:.0f} MiB load {int(row[4]) / slots:.3f}  spectrum / clean {s / min(clean):5.2f}")
        sweep[name] = (dev, offs, lens)
    if not a.no_merge_sweep:
        print("# VKIMG_SPECTRUM_MERGE at K 21, every 1: 0 a lane per window adds 1; 1 runs of equal keys in neighbouring lanes add "
              "once; 2 and equal keys anywhere in the wave instruction")
        for merge in (0, 1, 2):
            e2 = engine(merge)
            print(f"  merge {merge}: " + "  ".join(f"{name} {timed(e2, *sweep[name], 21, 1)[0] * 1e3:8.2f}" for name in work))
            e2.close()
    eng.close()


if __name__ == "__main__":
    main()
