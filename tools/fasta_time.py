#!/usr/bin/env python3
"""The FASTA count (vk_count_fasta_device) on a synthetic assembly generated in HBM: about --gbases Gbase of uniform ACGT
in 60-column lines, records of 1 to 50 Mbases under `>contigN ...` headers.  At k = 7 and k = 9: HIP events around each
of 10 timed launches after 3 warm-up launches (the context's workspaces are grown by then), median / min / max in
milliseconds, the text bytes read over the median as GB/s and as a fraction of the 8 TB/s HBM peak.  Beside each, as the
yardstick, the same bases as unwrapped FASTQ (one read per record) through the existing count in the same process --
and, at k = 7, through the classic kernel as well (a context made with VKIMG_K1_CLASSIC=1) -- with the same figures per
text byte of ITS text (about twice the bytes: a quality line per base).  Prints one JSON line per row and a table.

One process, one GPU; run it under a time limit:
    timeout -k 10 600 python tools/fasta_time.py
usage: python tools/fasta_time.py [--gbases G] [--reps R] [--warmup W] [--seed S] [--no-fastq]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12
WIDTH = 60


def record_lines(total_lines, seed):
    """Lines (of 60 bases) of each record: 1 to 50 Mbases, drawn until the total is used up."""
    rng = np.random.default_rng(seed)
    out, left = [], total_lines
    while left > 0:
        n = min(left, int(rng.integers(1_000_000 // WIDTH, 50_000_000 // WIDTH + 1)))
        out.append(n)
        left -= n
    return out


def synth(torch, device, gbases, seed):
    """(FASTA text, FASTQ text of the same bases unwrapped, bases): uint8 tensors on the device, 16 spare bytes behind."""
    total_lines = int(gbases * 1e9) // WIDTH
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    lines = torch.empty((total_lines, WIDTH + 1), dtype=torch.uint8, device=device)
    step = 1 << 22
    for at in range(0, total_lines, step):   # (in pieces: the intermediates of the arithmetic stay small)
        c = torch.randint(0, 4, (min(step, total_lines - at), WIDTH), dtype=torch.uint8, device=device, generator=g)
        lines[at:at + step, :WIDTH] = 65 + 2 * c + 2 * (c == 2).to(torch.uint8) + 13 * (c == 3).to(torch.uint8)   # A C G T
    lines[:, WIDTH] = 10
    recs = record_lines(total_lines, seed)
    tail = torch.zeros(16, dtype=torch.uint8, device=device)

    def text(s):
        return torch.frombuffer(bytearray(s), dtype=torch.uint8).to(device)
    fa, fq, at = [], [], 0
    for i, n in enumerate(recs):
        body = lines[at:at + n]
        fa += [text(b">contig%d length=%d synthetic\n" % (i, n * WIDTH)), body.reshape(-1)]
        fq += [text(b"@contig%d\n" % i), body[:, :WIDTH].reshape(-1), text(b"\n+\n"),
               torch.full((n * WIDTH,), 73, dtype=torch.uint8, device=device), text(b"\n")]
        at += n
    fasta = torch.cat(fa + [tail])
    fastq = torch.cat(fq + [tail])
    return fasta, fasta.numel() - 16, fastq, fastq.numel() - 16, total_lines * WIDTH, len(recs)


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


def row(name, k, nbytes, bases, ms):
    med = float(np.median(ms))
    r = {"what": name, "k": k, "text_bytes": nbytes, "bases": bases, "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
         "ms_max": round(max(ms), 3), "gb_per_s": round(nbytes / med / 1e6, 1), "of_hbm_peak": round(nbytes / (med * 1e-3) / PEAK_BYTES_PER_S, 4),
         "gbases_per_s": round(bases / med / 1e6, 2)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20260101)
    ap.add_argument("--no-fastq", action="store_true", help="skip the FASTQ yardstick")
    a = ap.parse_args()
    import torch
    from varkoder_amd.engine import ImageEngine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    fasta, fa_n, fastq, fq_n, bases, nrec = synth(torch, dev, a.gbases, a.seed)
    print(json.dumps({"records": nrec, "bases": bases, "fasta_bytes": fa_n, "fastq_bytes": fq_n, "warmup": a.warmup, "reps": a.reps,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    offs = np.zeros(1, dtype=np.uint64)
    rows = []
    for k in (7, 9):
        eng = ImageEngine(k=k, mapping="cgr", device=0)
        lens = np.array([fa_n], dtype=np.uint64)
        hist = torch.empty((1, 4 ** k), dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        nb = torch.empty(1, dtype=torch.int64, device=dev)
        ms = timed(torch, lambda: eng.count_fasta(fasta, offs, lens, hist, status, nb), a.warmup, a.reps)
        assert int(status.cpu()[0]) == 0 and int(nb.cpu()[0]) == bases
        rows.append(row("fasta", k, fa_n, bases, ms))
        fa_hist = hist.clone()
        if not a.no_fastq:
            qlens = np.array([fq_n], dtype=np.uint64)
            ms = timed(torch, lambda: eng.count(fastq, offs, qlens, 0, hist, status), a.warmup, a.reps)
            assert int(status.cpu()[0]) == 0 and torch.equal(hist, fa_hist), "the two counts differ"
            rows.append(row("fastq", k, fq_n, bases, ms))
            if k <= 7:
                os.environ["VKIMG_K1_CLASSIC"] = "1"
                try:
                    classic = ImageEngine(k=k, mapping="cgr", device=0)
                finally:
                    del os.environ["VKIMG_K1_CLASSIC"]
                ms = timed(torch, lambda: classic.count(fastq, offs, qlens, 0, hist, status), a.warmup, a.reps)
                assert torch.equal(hist, fa_hist)
                rows.append(row("fastq_classic", k, fq_n, bases, ms))
                classic.close()
        eng.close()
    print("| input | k | text bytes | median ms (min-max) | GB/s of text | of 8 TB/s | Gbases/s |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['what']} | {r['k']} | {r['text_bytes']} | {r['ms_median']} ({r['ms_min']}-{r['ms_max']}) | {r['gb_per_s']} | "
              f"{r['of_hbm_peak']:.2%} | {r['gbases_per_s']} |")


if __name__ == "__main__":
    main()
