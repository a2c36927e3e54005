#!/usr/bin/env python3
"""The per-window FASTA count (vk_count_fasta_windows_device) beside the whole-file count (vk_count_fasta_device) and the
per-record count (vk_count_fasta_records_device) in one process, on the synthetic texts of tools/fasta_records_time.py
(about --gbases Gbase of uniform ACGT in 60-column lines, generated in HBM):
    whole       count_fasta of the one-record text                                   k = 7, 9
    r5000       count_fasta_records of the same amount as records of 5,000 bases     k = 7 (all selected)
    w10000      windows of the one record at (N, S) = (10000, 10000)                 k = 7, 9
    w10000/4    the same at (10000, 2500): tiles of 2,500 bases, four to a window    k = 7
A window count runs over all its row ranges (fasta.window_plan with --max-hist-gib for rows and tile rows: at k = 9 a
row is 1 MiB and the rows of a chromosome do not fit in one call), one call per range into one buffer, and its time is
the sum over the ranges.  HIP events around each of --reps timed runs after --warmup warm-up runs (the context's
workspaces are grown by then), median / min / max in milliseconds.  Before timing, every row of a range is checked to
hold N k-mers (the text is all ACGT).  Prints one JSON line per row and a table; the comparison to record is w10000 at
k = 7 against r5000.

One process, one GPU; run it under a time limit:
    timeout -k 10 900 python tools/fasta_windows_time.py
usage: python tools/fasta_windows_time.py [--gbases G] [--reps R] [--warmup W] [--seed S] [--max-hist-gib M]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_records_time as RT  # noqa: E402


def stats(ms):
    return {"ms": round(float(np.median(ms)), 3), "min_max": [round(min(ms), 3), round(max(ms), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20260101)
    ap.add_argument("--max-hist-gib", type=float, default=16.0)
    a = ap.parse_args()
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine, _u64
    from varkoder_amd.fasta import window_plan
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    print(json.dumps({"gbases": a.gbases, "warmup": a.warmup, "reps": a.reps, "max_hist_gib": a.max_hist_gib,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    offs = np.zeros(1, dtype=np.uint64)
    budget = int(a.max_hist_gib * 2 ** 30)
    rows = []

    # the per-record figure the window count is compared with
    text, nbytes, bases, nrec = RT.synth_records(torch, dev, a.gbases, a.seed)
    lens = np.array([nbytes], dtype=np.uint64)
    k = 7
    eng = ImageEngine(k=k, mapping="cgr", device=0)
    rec_first, _, rec_bases, _, _ = eng.fasta_records(text, offs, lens)
    assert int(rec_first[1]) == nrec and int(rec_bases.sum()) == bases
    nsel = min(nrec, max(1, budget // (4 * 4 ** k)))
    slot = np.full(nrec, _capi.VK_FA_NO_SLOT, dtype=np.uint32)
    slot[:nsel] = np.arange(nsel, dtype=np.uint32)
    d_slot = torch.from_numpy(slot.view(np.int32)).to(dev)
    hist = torch.empty((nsel, 4 ** k), dtype=torch.int32, device=dev)
    o, ln = eng._desc(offs, lens)

    def per_record():
        st = eng.L.vk_count_fasta_records_device(eng.ctx, eng._ptr(text), _u64(o), _u64(ln), 1, k, _u64(rec_first), eng._ptr(d_slot),
                                                 nsel, eng._ptr(hist))
        _capi.check(eng.ctx, st, "vk_count_fasta_records_device")
    r = dict(what="r5000", k=k, bases=bases, rows=nsel, calls=1, **stats(RT.timed(torch, per_record, a.warmup, a.reps)))
    print(json.dumps(r), flush=True)
    rows.append(r)
    del hist, d_slot, text
    eng.close()
    torch.cuda.empty_cache()

    text, nbytes, bases, nrec = RT.synth_one(torch, dev, a.gbases, a.seed)
    lens = np.array([nbytes], dtype=np.uint64)
    for k, geometries in ((7, ((10000, 10000), (10000, 2500))), (9, ((10000, 10000),))):
        eng = ImageEngine(k=k, mapping="cgr", device=0)
        whole = torch.empty((1, 4 ** k), dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        nb = torch.empty(1, dtype=torch.int64, device=dev)
        r = dict(what="whole", k=k, bases=bases, rows=1, calls=1,
                 **stats(RT.timed(torch, lambda: eng.count_fasta(text, offs, lens, whole, status, nb), a.warmup, a.reps)))
        assert int(status.cpu()[0]) == 0 and int(nb.cpu()[0]) == bases
        print(json.dumps(r), flush=True)
        rows.append(r)
        rec_first, _, rec_bases, _, _ = eng.fasta_records(text, offs, lens)
        assert int(rec_first[1]) == 1 and int(rec_bases[0]) == bases
        d_bases = torch.from_numpy(np.ascontiguousarray(rec_bases).view(np.int64)).to(dev)
        for n, s in geometries:
            win_first, ranges = window_plan(rec_bases, n, s, hist_bytes=budget, ncode=4 ** k)
            d_first = torch.from_numpy(win_first.view(np.int64)).to(dev)
            hist = torch.empty((max(nr for _, nr, _ in ranges), 4 ** k), dtype=torch.int32, device=dev)

            def windows(check=False):
                for lo, nr, tiles in ranges:
                    eng.count_fasta_windows(text, offs, lens, rec_first, d_bases, d_first, n, s, lo, nr, tiles, hist=hist[:nr])
                    if check:
                        assert bool((hist[:nr].sum(dim=1, dtype=torch.int64) == n).all()), (lo, nr)
            windows(check=True)
            r = dict(what=f"w{n}" + ("" if s == n else f"/{n // s}"), k=k, bases=bases, rows=sum(nr for _, nr, _ in ranges),
                     calls=len(ranges), **stats(RT.timed(torch, windows, a.warmup, a.reps)))
            print(json.dumps(r), flush=True)
            rows.append(r)
            del hist
            torch.cuda.empty_cache()
        eng.close()
    ms = {(r["what"], r["k"]): r["ms"] for r in rows}
    print("| what | k | rows | calls | ms (min-max) | against whole, same k | against r5000, k = 7 |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['what']} | {r['k']} | {r['rows']} | {r['calls']} | {r['ms']} ({r['min_max'][0]}-{r['min_max'][1]}) | "
              f"{r['ms'] / ms[('whole', r['k'])]:.2f} | {r['ms'] / ms[('r5000', 7)] if r['k'] == 7 else float('nan'):.2f} |")


if __name__ == "__main__":
    main()
