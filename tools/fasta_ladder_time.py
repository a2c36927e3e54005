#!/usr/bin/env python3
"""The subsample ladder of an assembly (vk_count_fasta_sampled_device, `image --from-fasta --fragments`) on the synthetic
assembly of tools/fasta_time.py (about --gbases Gbase in 60-column lines).  At k = 7 and k = 9, in one process: the whole
count (count_fasta) and the nine-step ladder 200M ... 500K of that sample in ONE count_fasta_sampled call (fragments of
--fragment-length bases; the plan is fasta.fasta_plan's), HIP events around each of --reps timed calls after --warmup
warm-up calls; then each step in a call of its own, which shows what the index costs (every call builds it) and how a
step's time falls with the share of the fragments it takes.  Prints one JSON line per row and a table; the ladder's time
as a multiple of the whole count's is the figure DESIGN.md quotes.

One process, one GPU; run it under a time limit:
    timeout -k 10 600 python tools/fasta_ladder_time.py
usage: python tools/fasta_ladder_time.py [--gbases G] [--fragment-length L] [--reps R] [--warmup W] [--seed S]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fasta_time import synth, timed  # noqa: E402


def row(what, k, steps, ms, whole_ms=None, taken=None):
    med = float(np.median(ms))
    r = {"what": what, "k": k, "steps": steps, "ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
    if whole_ms is not None:
        r["of_whole_count"] = round(med / whole_ms, 3)
    if taken is not None:
        r["taken"] = taken
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--fragment-length", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20260101)
    a = ap.parse_args()
    import torch
    from varkoder_amd.engine import ImageEngine
    from varkoder_amd.fasta import fasta_plan
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    fasta, fa_n, _, _, bases, nrec = synth(torch, dev, a.gbases, a.seed)
    L = a.fragment_length
    max_bp = 200_000_000 if bases > 200_000_000 else bases // 5   # (smaller with a smaller --gbases: nine steps all the same)
    _, steps = fasta_plan([bases], [0], L, seed=a.seed, min_bp=max_bp // 400, max_bp=max_bp)
    sizes = [st[2] for st in steps]
    print(json.dumps({"records": nrec, "bases": bases, "fasta_bytes": fa_n, "fragment_length": L, "ladder": sizes, "warmup": a.warmup,
                      "reps": a.reps, "device": torch.cuda.get_device_name(0)}), flush=True)
    offs, lens = np.zeros(1, dtype=np.uint64), np.array([fa_n], dtype=np.uint64)
    rows = []
    for k in (7, 9):
        eng = ImageEngine(k=k, mapping="cgr", device=0)
        hist = torch.empty((1, 4 ** k), dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        nb = torch.empty(1, dtype=torch.int64, device=dev)
        ms = timed(torch, lambda: eng.count_fasta(fasta, offs, lens, hist, status, nb), a.warmup, a.reps)
        assert int(status.cpu()[0]) == 0 and int(nb.cpu()[0]) == bases
        whole = row("whole count", k, 1, ms)
        rows.append(whole)

        def ladder(part):
            return eng.count_fasta_sampled(fasta, offs, lens, L, [0] * len(part), [st[3] for st in part], [st[4] for st in part],
                                           [st[5] for st in part])
        ms = timed(torch, lambda: ladder(steps), a.warmup, a.reps)
        h, st_, nb2, taken = ladder(steps)
        assert int(st_.cpu()[0]) == 0 and int(nb2.cpu()[0]) == bases
        taken = taken.cpu().tolist()
        windows = h.to(torch.int64).sum(dim=1).cpu().tolist()
        for bp, t, w in zip(sizes, taken, windows):   # (a taken fragment of L bases holds at most L - k + 1 windows)
            assert abs(t - bp) < 0.05 * bp + 50 * L and 0 < w <= t, (bp, t, w)
        rows.append(row("ladder, one call", k, len(steps), ms, whole["ms_median"], taken))
        for st in steps:
            ms = timed(torch, lambda: ladder([st]), 1, max(3, a.reps // 2))
            rows.append(row("step %d alone" % st[2], k, 1, ms, whole["ms_median"]))
        eng.close()
    print("| what | k | steps | median ms (min-max) | of the whole count |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['what']} | {r['k']} | {r['steps']} | {r['ms_median']} ({r['ms_min']}-{r['ms_max']}) | {r.get('of_whole_count', 1)} |")


if __name__ == "__main__":
    main()
