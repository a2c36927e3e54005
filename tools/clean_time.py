#!/usr/bin/env python3
"""Step B's kernels (vk_clean_device) on one large paired sample: 1M pairs x 150 bp by default (~0.6 GB of raw
text), with the shapes of tests/clean_ref.synth_set (fragments shorter and longer than the reads, adapters, poly-G,
N bases, 10 % duplicates), generated with numpy here and uploaded once.  Prints one JSON line: the clean call's
time (best of --reps, device-synchronised), GB/s of raw text, and the time of each other stage of a sample's
`--from-raw` path in the same process -- upload (H2D), line count, ladder + images -- so that step B's share of
the wall time can be read off.  Under `rocprofv3 --kernel-trace --stats -- python tools/clean_time.py` the
per-kernel times come from the trace.

--single-end cleans the R1 text alone, as one file of single reads.  --detect-adapters times adapter detection
(vk_clean_detect_device) plus the clean with trimming by sequence (vk_clean_adapters_device) as one call, and adds
the detection's own time and what it found to the line.

usage: python tools/clean_time.py [--pairs N] [--len L] [--reps R] [--single-end] [--detect-adapters]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADAPTER1 = np.frombuffer(b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", dtype=np.uint8)
ADAPTER2 = np.frombuffer(b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT", dtype=np.uint8)


def make_pairs(n, L, seed=1):
    """(R1 text, R2 text) of n pairs: fixed-size records `@pNNNNNNNN 1:N:0\\n<L>\\n+\\n<L>\\n`."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGTN")] = list(b"TGCAN")
    span = 2 * L + 100
    frag = acgt[rng.integers(0, 4, (n, span))]
    frag[rng.random((n, span)) < 0.003] = ord("N")
    ins = np.where(rng.random(n) < 0.3, rng.integers(40, L, n), rng.integers(L + 1, span, n))
    dup = np.flatnonzero(rng.random(n) < 0.1)
    frag[dup] = frag[rng.integers(0, n, len(dup))]
    ins[dup] = L + 50
    pos = np.arange(L)[None, :]
    r1 = frag[:, :L].copy()
    # R2: reverse complement of the fragment's first `ins` bases, read from its end
    idx = ins[:, None] - 1 - pos
    r2 = comp[np.take_along_axis(frag, np.clip(idx, 0, span - 1), axis=1)]
    for r, ad in ((r1, ADAPTER1), (r2, ADAPTER2)):
        past = pos - ins[:, None]                              # >= 0: into the adapter, then poly-G
        r[:] = np.where(past < 0, r, np.where(past < len(ad), ad[np.clip(past, 0, len(ad) - 1)], ord("G")))
    out = []
    for mate, r in ((1, r1), (2, r2)):
        head = np.frombuffer(b"".join(b"@p%08d %d:N:0\n" % (i, mate) for i in range(n)), dtype=np.uint8).reshape(n, -1)
        qual = (rng.integers(0, 41, (n, L)) + 33).astype(np.uint8)
        nl = np.full((n, 1), ord("\n"), dtype=np.uint8)
        plus = np.frombuffer(b"\n+\n", dtype=np.uint8)[None, :].repeat(n, axis=0)
        out.append(np.concatenate([head, r, plus, qual, nl], axis=1).ravel())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-end", action="store_true", help="the R1 text alone, as single reads")
    ap.add_argument("--detect-adapters", action="store_true", help="detection + trimming by sequence in the timed call")
    a = ap.parse_args()
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import ImageEngine
    from varkoder_amd.subsample import ladder_counts
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    r1, r2 = make_pairs(a.pairs, a.len)
    texts = [r1] if a.single_end else [r1, r2]
    raw = sum(len(x) for x in texts)
    sync = torch.cuda.synchronize
    t = time.perf_counter()
    dev, offs, lens = eng.upload(texts)
    sync()
    t_upload = time.perf_counter() - t
    t = time.perf_counter()
    lines = eng.clean_lines(dev, offs, lens)
    t_lines = time.perf_counter() - t
    recs = lines // 4
    roles, owner = ([_capi.VK_CL_ROLE_UNPAIRED], [0]) if a.single_end else ([_capi.VK_CL_ROLE_R1, _capi.VK_CL_ROLE_R2], [0, 0])
    best, detect, extra, found = [], [], {}, None
    for _ in range(a.reps):
        sync()
        t = time.perf_counter()
        if a.detect_adapters:
            found = eng.detect_adapters(dev, offs, lens, recs, roles, owner, 1)
            detect.append(time.perf_counter() - t)
        out, oo, ol, st, status, *rest = eng.clean(dev, offs, lens, recs, roles, owner, 1, adapters=found)   # (waits for the kernels)
        best.append(time.perf_counter() - t)
    assert not status.any(), status
    if a.detect_adapters:
        ast = rest[0]
        extra = {"detect_s_best": min(detect), "detect_s_all": detect,
                 "adapters": [x.decode() if x is not None else None for x in found[0]],
                 "adapter_trimmed_reads": int(ast[0][0]), "adapter_trimmed_bases": int(ast[0][1])}
    if a.single_end:
        extra["single_end"] = True
    sync()
    t = time.perf_counter()
    rec = ladder_counts(eng, out, oo, ol, seed=1, min_bp=500000, max_bp=200_000_000)[0]
    imgs = eng.images(torch.stack([h for _, h, _ in rec["steps"]]))
    sync()
    t_ladder = time.perf_counter() - t
    clean_s = min(best)
    total = t_upload + t_lines + clean_s + t_ladder
    print(json.dumps({
        "pairs": a.pairs, "read_len": a.len, "raw_bytes": raw, "clean_out_bytes": int(ol[0]), "records_out": int(st[0][1]),
        "clean_s_best": clean_s, "clean_s_all": best, "clean_gb_s": raw / clean_s / 1e9,
        "upload_s": t_upload, "upload_gb_s": raw / t_upload / 1e9, "lines_s": t_lines, "ladder_images_s": t_ladder,
        "ladder_steps": len(rec["steps"]), "images": int(imgs.shape[0]),
        "clean_share_of_device_path": clean_s / total, **extra}))
    eng.close()


if __name__ == "__main__":
    main()
