#!/usr/bin/env python3
"""The per-record FASTA count (vk_count_fasta_records_device) beside the whole-file count (vk_count_fasta_device) on the
same text, in the same process: a synthetic text of about --gbases Gbase of uniform ACGT in 60-column lines, generated
in HBM, in two shapes --
    one      one record: every workgroup but the first is entered by it (k <= 7: all on the LDS table)
    r5000    records of 5,000 bases under `>NNNNNNN` headers, all selected: a header about every 80 lanes, nearly all
             windows on rows in HBM
At k = 7 and k = 9: HIP events around each of --reps timed calls after --warmup warm-up calls (the context's workspaces
are grown by then), median / min / max in milliseconds, and the ratio of the medians.  The rows of one call are held to
--max-hist-gib of HBM: where all records of r5000 do not fit (k = 9: 1 MiB a row), the first that do are selected and
the rest of the text is skipped by the kernel, and the row says how many were counted.  Before timing, the sum of the
rows is checked against the whole-file row.  Prints one JSON line per row and a table.

One process, one GPU; run it under a time limit:
    timeout -k 10 600 python tools/fasta_records_time.py
usage: python tools/fasta_records_time.py [--gbases G] [--reps R] [--warmup W] [--seed S] [--max-hist-gib M]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTH = 60
RECORD = 5000


def bases_matrix(torch, device, rows, cols, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    step = max(1, (1 << 28) // cols)
    for at in range(0, rows, step):   # (in pieces: the intermediates of the arithmetic stay small)
        c = torch.randint(0, 4, (min(step, rows - at), cols), dtype=torch.uint8, device=device, generator=g)
        out[at:at + step] = 65 + 2 * c + 2 * (c == 2).to(torch.uint8) + 13 * (c == 3).to(torch.uint8)   # A C G T
    return out


def synth_one(torch, device, gbases, seed):
    """(text with 16 spare bytes behind, its length, bases, records): one record in 60-column lines."""
    nlines = int(gbases * 1e9) // WIDTH
    lines = torch.empty((nlines, WIDTH + 1), dtype=torch.uint8, device=device)
    lines[:, :WIDTH] = bases_matrix(torch, device, nlines, WIDTH, seed)
    lines[:, WIDTH] = 10
    head = torch.frombuffer(bytearray(b">chr1 synthetic\n"), dtype=torch.uint8).to(device)
    text = torch.cat([head, lines.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=device)])
    return text, text.numel() - 16, nlines * WIDTH, 1


def synth_records(torch, device, gbases, seed):
    """The same amount in records of RECORD bases: `>NNNNNNN\\n`, 83 lines of 60 and one of 20."""
    nrec = int(gbases * 1e9) // RECORD
    full, rest = RECORD // WIDTH, RECORD % WIDTH
    b = bases_matrix(torch, device, nrec, RECORD, seed)
    block = torch.empty((nrec, 9 + full * (WIDTH + 1) + rest + 1), dtype=torch.uint8, device=device)
    block[:, 0] = 62
    idx = torch.arange(nrec, device=device)
    for j in range(7):
        block[:, 7 - j] = (48 + (idx // 10 ** j) % 10).to(torch.uint8)
    block[:, 8] = 10
    body = block[:, 9:9 + full * (WIDTH + 1)].unflatten(1, (full, WIDTH + 1))   # (a view)
    body[:, :, :WIDTH] = b[:, :full * WIDTH].reshape(nrec, full, WIDTH)
    body[:, :, WIDTH] = 10
    block[:, 9 + full * (WIDTH + 1):-1] = b[:, full * WIDTH:]
    block[:, -1] = 10
    text = torch.cat([block.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=device)])
    return text, text.numel() - 16, nrec * RECORD, nrec


def timed(torch, call, warmup, reps):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20260101)
    ap.add_argument("--max-hist-gib", type=float, default=16.0)
    a = ap.parse_args()
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine, _u64
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    print(json.dumps({"gbases": a.gbases, "warmup": a.warmup, "reps": a.reps, "max_hist_gib": a.max_hist_gib,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    offs = np.zeros(1, dtype=np.uint64)
    rows = []
    for shape, synth in (("one", synth_one), ("r5000", synth_records)):
        text, nbytes, bases, nrec = synth(torch, dev, a.gbases, a.seed)
        lens = np.array([nbytes], dtype=np.uint64)
        for k in (7, 9):
            eng = ImageEngine(k=k, mapping="cgr", device=0)
            whole = torch.empty((1, 4 ** k), dtype=torch.int32, device=dev)
            status = torch.empty(1, dtype=torch.int32, device=dev)
            nb = torch.empty(1, dtype=torch.int64, device=dev)
            ms_whole = timed(torch, lambda: eng.count_fasta(text, offs, lens, whole, status, nb), a.warmup, a.reps)
            assert int(status.cpu()[0]) == 0 and int(nb.cpu()[0]) == bases
            rec_first, _, rec_bases, _, _ = eng.fasta_records(text, offs, lens)
            assert int(rec_first[1]) == nrec and int(rec_bases.sum()) == bases
            nsel = min(nrec, max(1, int(a.max_hist_gib * 2 ** 30) // (4 * 4 ** k)))
            slot = np.full(nrec, _capi.VK_FA_NO_SLOT, dtype=np.uint32)
            slot[:nsel] = np.arange(nsel, dtype=np.uint32)
            d_slot = torch.from_numpy(slot.view(np.int32)).to(dev)
            hist = torch.empty((nsel, 4 ** k), dtype=torch.int32, device=dev)
            o, ln = eng._desc(offs, lens)

            def call():
                st = eng.L.vk_count_fasta_records_device(eng.ctx, eng._ptr(text), _u64(o), _u64(ln), 1, k, _u64(rec_first),
                                                         eng._ptr(d_slot), nsel, eng._ptr(hist))
                _capi.check(eng.ctx, st, "vk_count_fasta_records_device")
            ms = timed(torch, call, a.warmup, a.reps)
            if nsel == nrec:
                assert torch.equal(hist.sum(dim=0, dtype=torch.int64) & 0xFFFFFFFF, whole[0].long() & 0xFFFFFFFF), "the rows do not sum to the file's"
            med, med_whole = float(np.median(ms)), float(np.median(ms_whole))
            r = {"shape": shape, "k": k, "text_bytes": nbytes, "bases": bases, "records": nrec, "records_counted": nsel,
                 "per_record_ms": round(med, 3), "per_record_min_max": [round(min(ms), 3), round(max(ms), 3)],
                 "count_fasta_ms": round(med_whole, 3), "count_fasta_min_max": [round(min(ms_whole), 3), round(max(ms_whole), 3)],
                 "ratio": round(med / med_whole, 3)}
            print(json.dumps(r), flush=True)
            rows.append(r)
            del hist, d_slot
            eng.close()
        del text
        torch.cuda.empty_cache()
    print("| shape | k | records counted | per-record ms (min-max) | count_fasta ms (min-max) | ratio |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['shape']} | {r['k']} | {r['records_counted']} of {r['records']} | {r['per_record_ms']} "
              f"({r['per_record_min_max'][0]}-{r['per_record_min_max'][1]}) | {r['count_fasta_ms']} "
              f"({r['count_fasta_min_max'][0]}-{r['count_fasta_min_max'][1]}) | {r['ratio']} |")


if __name__ == "__main__":
    main()
