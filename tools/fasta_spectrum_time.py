#!/usr/bin/env python3
"""The assemblies' k-mer spectrum (vk_spectrum_fasta_device) on tools/fasta_time.py's synthetic assembly generated in HBM
(--gbases Gbase, 0.5 by default: under the screen's 1 GiB cap, so that the baseline runs), K = 21, every = 1, against the two
kernels that do the nearest job, in one process, the legs taken in turn within every repeat:
    a  vk_spectrum_fasta_device: FASTA text -> counting table
    b  vk_screen_build_device (ImageEngine.screen_set's call) on the same text with the same number of slots: the same keys
       inserted, no counts kept, the text read a byte at a time
    c  vk_spectrum_device on the same bases written as 150-base FASTQ reads, with the same slots
HIP events around each of --reps timed calls after --warmup warm-up rounds; per leg the median / min / max in milliseconds,
windows/s (the leg's own windows over the median) and GB/s of its text.  Prints one JSON line per leg and a table.
(a) and (c) must agree with themselves between repeats; (a)'s distinct keys must equal (b)'s.

One process, one GPU; run it under a time limit.  For a kernel trace run leg a alone in a run of its own:
    timeout -k 10 600 python tools/fasta_spectrum_time.py
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/fasta_spectrum_time.py --legs a --reps 3 --warmup 1
--tandem-fraction F overwrites the bases of the first F of the text with the 7-base tandem repeat (ACGGTCA)n -- a satellite:
seven keys, no two consecutive windows equal, so a lane's fold of equal consecutive keys does not see it and every lane of
every wave adds to the same seven slots.  What it costs is what a wave-level merge would have to win back.
usage: python tools/fasta_spectrum_time.py [--gbases G] [--reps R] [--warmup W] [--seed S] [--legs a,b,c] [--tandem-fraction F]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_time  # noqa: E402

K, EVERY, READ = 21, 1, 150


def reads_of(torch, fasta, n):
    """The assembly's bases (its upper-case ACGT: the headers are lower case) as FASTQ text of 150-base reads."""
    t = fasta[:n]
    bases = t[(t == 65) | (t == 67) | (t == 71) | (t == 84)]
    nreads = bases.numel() // READ
    rec = torch.empty((nreads, 2 * READ + 7), dtype=torch.uint8, device=fasta.device)
    rec[:, 0], rec[:, 1], rec[:, 2] = 64, 114, 10                      # "@r\n"
    rec[:, 3:3 + READ] = bases[:nreads * READ].reshape(nreads, READ)
    rec[:, 3 + READ], rec[:, 4 + READ], rec[:, 5 + READ] = 10, 43, 10  # "\n+\n"
    rec[:, 6 + READ:6 + 2 * READ] = 73
    rec[:, 6 + 2 * READ] = 10
    text = torch.cat([rec.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=fasta.device)])
    return text, text.numel() - 16, nreads


def tandem(torch, fasta, n, fraction):
    """The bases of the first `fraction` of the text become (ACGGTCA)n; the headers and line ends stay."""
    cut = int(n * fraction)
    head = fasta[:cut]
    mask = (head == 65) | (head == 67) | (head == 71) | (head == 84)
    ordinal = torch.cumsum(mask, 0)[mask] - 1
    unit = torch.frombuffer(bytearray(b"ACGGTCA"), dtype=torch.uint8).to(fasta.device)
    head[mask] = unit[ordinal % 7]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20260101)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--tandem-fraction", type=float, default=0.0)
    a = ap.parse_args()
    legs = a.legs.split(",")
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine, _u64
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    fasta, fa_n, _, _, bases, nrec = fasta_time.synth(torch, dev, a.gbases, a.seed)
    if a.tandem_fraction > 0:
        tandem(torch, fasta, fa_n, a.tandem_fraction)
    eng = ImageEngine(k=7, mapping="cgr", device=0)   # (the image's k and mapping are not used)
    nslots = eng.spectrum_fasta_slots(fa_n, EVERY)
    print(json.dumps({"records": nrec, "bases": bases, "fasta_bytes": fa_n, "slots": nslots, "k": K, "every": EVERY,
                      "tandem_fraction": a.tandem_fraction, "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)}), flush=True)
    keys = torch.empty(nslots, dtype=torch.int64, device=dev)
    counts = torch.empty(nslots, dtype=torch.int32, device=dev)
    rows = torch.empty((1, _capi.VK_SPEC_NSTAT), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    offs, base, nsl = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.array([nslots], dtype=np.uint64)
    fa_lens = np.array([fa_n], dtype=np.uint64)
    calls, nbytes, result = {}, {}, {}

    def workspace(fn, *args):
        n = C.c_uint64()
        _capi.check(eng.ctx, fn(*args, C.byref(n)), "workspace size")
        return torch.empty(max(int(n.value), 256), dtype=torch.uint8, device=dev)

    if "a" in legs:
        ws_a = workspace(eng.L.vk_spectrum_fasta_workspace_size, _u64(fa_lens), 1)

        def leg_a():
            st = eng.L.vk_spectrum_fasta_device(eng.ctx, eng._ptr(fasta), _u64(offs), _u64(fa_lens), 1, K, EVERY, eng._ptr(keys),
                                                eng._ptr(counts), _u64(base), _u64(nsl), eng._ptr(rows), eng._ptr(status),
                                                eng._ptr(ws_a), ws_a.numel())
            _capi.check(eng.ctx, st, "vk_spectrum_fasta_device")

        def res_a():
            r = rows.cpu().numpy().view(np.uint64)[0]
            assert int(status.cpu()[0]) == 0 and int(r[1]) == bases
            return int(r[2]), int(r[4])
        calls["a"], nbytes["a"], result["a"] = leg_a, fa_n, res_a
    if "b" in legs:
        ws_b = workspace(eng.L.vk_screen_build_workspace_size, fa_n)
        win_b, dis_b, st_b = C.c_uint64(), C.c_uint64(), C.c_uint32()

        def leg_b():   # (the call synchronises: its windows and distinct keys are the host's)
            st = eng.L.vk_screen_build_device(eng.ctx, eng._ptr(fasta), fa_n, K, eng._ptr(keys), nslots, eng._ptr(ws_b), ws_b.numel(),
                                              C.byref(win_b), C.byref(dis_b), C.byref(st_b))
            _capi.check(eng.ctx, st, "vk_screen_build_device")
        calls["b"], nbytes["b"], result["b"] = leg_b, fa_n, lambda: (int(win_b.value), int(dis_b.value))
    if "c" in legs:
        fastq, fq_n, nreads = reads_of(torch, fasta, fa_n)
        fq_lens, recs = np.array([fq_n], dtype=np.uint64), np.array([nreads], dtype=np.uint64)
        ws_c = workspace(eng.L.vk_spectrum_workspace_size, _u64(recs), 1, _u64(fq_lens))

        def leg_c():
            st = eng.L.vk_spectrum_device(eng.ctx, eng._ptr(fastq), _u64(offs), _u64(fq_lens), _u64(recs), 1, K, EVERY,
                                          eng._ptr(keys), eng._ptr(counts), _u64(base), _u64(nsl), eng._ptr(rows),
                                          eng._ptr(status), eng._ptr(ws_c), ws_c.numel())
            _capi.check(eng.ctx, st, "vk_spectrum_device")

        def res_c():
            r = rows.cpu().numpy().view(np.uint64)[0]
            assert int(status.cpu()[0]) == 0 and int(r[0]) == nreads
            return int(r[2]), int(r[4])
        calls["c"], nbytes["c"], result["c"] = leg_c, fq_n, res_c
    ms = {leg: [] for leg in calls}
    seen = {}
    for rep in range(a.warmup + a.reps):
        for leg, call in calls.items():   # the legs in turn within every repeat
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            got = result[leg]()
            assert seen.setdefault(leg, got) == got, f"leg {leg} differs between repeats"
            if rep >= a.warmup:
                ms[leg].append(e0.elapsed_time(e1))
    if "a" in seen and "b" in seen:
        assert seen["a"] == seen["b"], "the spectrum's windows and distinct keys are not the screen's"
    out = []
    for leg, v in ms.items():
        med = float(np.median(v))
        windows, distinct = seen[leg]
        r = {"leg": leg, "text_bytes": nbytes[leg], "windows": windows, "distinct": distinct, "ms_median": round(med, 3),
             "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "gwindows_per_s": round(windows / med / 1e6, 3),
             "gwindows_per_s_at_min_max": [round(windows / max(v) / 1e6, 3), round(windows / min(v) / 1e6, 3)],
             "gb_per_s": round(nbytes[leg] / med / 1e6, 2)}
        print(json.dumps(r), flush=True)
        out.append(r)
    print("| leg | text bytes | windows | median ms (min-max) | Gwindows/s (at max-min ms) | GB/s of text |")
    print("|---|---|---|---|---|---|")
    for r in out:
        print(f"| {r['leg']} | {r['text_bytes']} | {r['windows']} | {r['ms_median']} ({r['ms_min']}-{r['ms_max']}) | "
              f"{r['gwindows_per_s']} ({r['gwindows_per_s_at_min_max'][0]}-{r['gwindows_per_s_at_min_max'][1]}) | {r['gb_per_s']} |")
    eng.close()


if __name__ == "__main__":
    main()
