#!/usr/bin/env python3
"""The read screen (vk_screen_build_device, vk_screen_device: `--exclude-fasta` / `--keep-fasta`) on tools/clean_time.py's
workload: 1M pairs x 150 bp by default, cleaned on the GPU here, and the cleaned text screened against synthetic
references of 5,386 bases, 150 kb and 16 Mb (random sequence, wrapped at 70), at 0 % and at 10 % matching reads, in both
modes.  For the 10 % runs every tenth raw pair is cut from the reference (R1 forward, R2 the reverse complement of a
stretch nearby) before the upload, so each reference has its own cleaned text.  Prints, per reference, the time of the
build (the count pass and the insertion together) and, per run, the screen's time (best of --reps, device-synchronised)
beside vk_clean_device's time on the same reads, measured in the same run, and their ratio.  Under `rocprofv3
--kernel-trace --stats -- python tools/screen_time.py` the per-kernel times come from the trace.

usage: python tools/screen_time.py [--pairs N] [--len L] [--reps R] [--k K] [--refs 5386,150000,16000000]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from clean_time import make_pairs  # noqa: E402

HEAD = len(b"@p00000000 1:N:0\n")


def fasta_of(seq, width=70):
    full = len(seq) // width
    body = np.full((full, width + 1), ord("\n"), dtype=np.uint8)
    body[:, :width] = seq[:full * width].reshape(full, width)
    tail = seq[full * width:].tobytes()
    return b">synthetic reference\n" + body.tobytes() + (tail + b"\n" if tail else b"")


def plant(r1, r2, L, ref, rng, every=10):
    """Copies of the texts with every `every`-th pair cut from ref."""
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    out = []
    n = len(r1) // (HEAD + 2 * L + 4)
    rows = np.arange(0, n, every)
    p = rng.integers(0, max(1, len(ref) - 2 * L), len(rows))
    at = p[:, None] + np.arange(L)[None, :]
    fwd = ref[at % len(ref)]
    rev = comp[ref[(at + L // 2) % len(ref)]][:, ::-1]
    for text, seq in ((r1, fwd), (r2, rev)):
        t = text.reshape(n, -1).copy()
        t[rows, HEAD:HEAD + L] = seq
        out.append(t.ravel())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--refs", default="5386,150000,16000000")
    a = ap.parse_args()
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(3)
    r1, r2 = make_pairs(a.pairs, a.len)
    roles, owner = [_capi.VK_CL_ROLE_R1, _capi.VK_CL_ROLE_R2], [0, 0]

    def cleaned(texts):
        dev, offs, lens = eng.upload(texts)
        recs = eng.clean_lines(dev, offs, lens) // 4
        best = []
        for _ in range(a.reps):
            sync()
            t = time.perf_counter()
            out, oo, ol, st, status, *_ = eng.clean(dev, offs, lens, recs, roles, owner, 1)   # (waits for the kernels)
            best.append(time.perf_counter() - t)
        assert not status.any(), status
        return out, oo, ol, [int(st[0][1])], min(best)

    print(f"# {a.pairs} pairs x {a.len} bp, k = {a.k}, best of {a.reps}; times in ms")
    plain = cleaned([r1, r2])
    for nref in (int(x) for x in a.refs.split(",")):
        ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, nref)]
        fasta = fasta_of(ref)
        fdev, _, flens = eng.upload([fasta])
        build = []
        for _ in range(a.reps):
            sync()
            t = time.perf_counter()
            sset = eng.screen_set(fdev, int(flens[0]), a.k)   # (synchronises)
            build.append(time.perf_counter() - t)
        print(f"reference {nref} bases: {sset.distinct} distinct keys in {sset.slots} slots ({sset.slots * 8 / 2**20:.1f} MiB), "
              f"build {min(build) * 1e3:.2f}")
        for pct, work in ((0, plain), (10, None)):
            if work is None:
                work = cleaned(plant(r1, r2, a.len, ref, rng))
            out, oo, ol, recs, clean_s = work
            for keep in (False, True):
                best = []
                for _ in range(a.reps):
                    sync()
                    t = time.perf_counter()
                    _, _, slens, stats, status = eng.screen(out, oo, ol, sset, keep=keep, records=recs)   # (waits for the kernels)
                    best.append(time.perf_counter() - t)
                assert not status.any(), status
                s = stats[0]
                print(f"  {pct:2d} % planted, {'keep   ' if keep else 'exclude'}: screen {min(best) * 1e3:8.2f}  clean {clean_s * 1e3:8.2f}  "
                      f"screen / clean {min(best) / clean_s:5.2f}  reads in {int(s[0])} kept {int(s[1])} "
                      f"({100 * (int(s[0]) - int(s[1])) / max(1, int(s[0])):.1f} % removed), text {int(ol[0])} -> {int(slens[0])} bytes")
            del work, out
        del sset, fdev
    eng.close()


if __name__ == "__main__":
    main()
