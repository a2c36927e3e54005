#!/usr/bin/env python3
"""`--qc-report`'s call (vk_qc_device, ImageEngine.qc) beside step B's (vk_clean_device) on the workload of
tools/clean_time.py -- 1M pairs x 150 bp by default, ~0.6 GB of raw text -- in one process: the QC of the raw texts (R1
and R2 as two streams, every record), the cleaning, and the QC of the cleaned text.  Synchronised wall time of the engine
calls, best of --reps; each QC time also as bytes of text per second and as a share of the 6.3 TB/s that HBM gives a
streaming kernel on an MI355X.  Under `rocprofv3 --kernel-trace --stats -- python tools/qc_time.py --reps 1` the per-kernel
times come from the trace.

usage: python tools/qc_time.py [--pairs N] [--len L] [--reps R]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_ACHIEVABLE = 6.3e12   # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from clean_time import make_pairs
    from varkoder_amd import _capi, qc
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    r1, r2 = make_pairs(a.pairs, a.len)
    raw = len(r1) + len(r2)
    sync = torch.cuda.synchronize
    dev, offs, lens = eng.upload([r1, r2])
    recs = eng.clean_lines(dev, offs, lens) // 4
    roles, owner = [_capi.VK_CL_ROLE_R1, _capi.VK_CL_ROLE_R2], [0, 0]

    def best(call):
        times, got = [], None
        for _ in range(a.reps):
            sync()
            t = time.perf_counter()
            got = call()   # (waits for the kernels: its results come back to the host)
            times.append(time.perf_counter() - t)
        return min(times), got

    t_clean, (out, oo, ol, st, status, *_) = best(lambda: eng.clean(dev, offs, lens, recs, roles, owner, 1))
    assert not status.any(), status
    out_recs = np.array([st[0][1]], dtype=np.uint64)
    t_raw, (rows_raw, st_raw) = best(lambda: eng.qc(dev, offs, lens, recs))
    t_after, (rows_after, st_after) = best(lambda: eng.qc(out, oo, ol, out_recs))
    assert not st_raw.any() and not st_after.any()
    before, after = qc.totals(qc.add_rows(rows_raw)), qc.totals(rows_after[0])
    assert before["total_reads"] == 2 * a.pairs and after["total_reads"] == int(out_recs[0])
    cleaned = int(ol[0])
    print(f"# {a.pairs} pairs x {a.len} bp, best of {a.reps}; times in ms")
    print(f"clean (vk_clean_device)      {t_clean * 1e3:8.2f}  {raw} bytes of raw text -> {cleaned} bytes, {int(out_recs[0])} reads")
    for name, t, nbytes in (("qc of the raw texts  ", t_raw, raw), ("qc of the cleaned text", t_after, cleaned)):
        rate = nbytes / t
        print(f"{name}       {t * 1e3:8.2f}  {rate / 1e9:7.1f} GB/s of text = {rate / HBM_ACHIEVABLE:.3f} of 6.3 TB/s"
              f"  ({t / t_clean:.2f} of the cleaning)")
    print(f"both qc calls / clean        {(t_raw + t_after) / t_clean:8.2f}")
    print(f"raw:   reads {before['total_reads']} bases {before['total_bases']} q30 {before['q30_rate']:.4f} gc {before['gc_content']:.4f}")
    print(f"clean: reads {after['total_reads']} bases {after['total_bases']} q30 {after['q30_rate']:.4f} gc {after['gc_content']:.4f}"
          f" mean length {after['mean_length']:.1f}")
    eng.close()


if __name__ == "__main__":
    main()
