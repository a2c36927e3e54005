#!/usr/bin/env python3
"""`--from-bam`'s conversion (vk_bam_frame_device, vk_bam_fastq_device) on synthetic unaligned BAMs, beside the stages
around it in the same process: 1M reads x 150 bases (short reads) and 10,000 reads x 15,000 bases (long reads) by
default, each generated with numpy here, written as BGZF (zlib level 1, members of 0xFF00 bytes) to a temporary file and
brought in the way the commands bring it in (ImageEngine.stage_files + upload_staged: read, copy, inflate in HBM).

Prints one JSON line per input: the upload's wall time and the part of it spent in the inflate call; bam_frame and
bam_fastq (best of --reps after a warm-up call, the calls synchronise; bam_fastq frames again before it emits, so emit
alone is about bam_fastq - bam_frame), both also with VK_BAM_NO_GUESS; the segments and how many the link pass walked
again; and ImageEngine.clean_lines + clean on the converted text, as `--from-raw` runs them behind the conversion.
Under `rocprofv3 --kernel-trace --stats -- python tools/bam_time.py` the per-kernel times come from the trace.

--groups N[,N...]: for each N the short-read file is written again with N @RG lines and an `RG:Z:` field of fixed size in
every record (the groups dealt pseudo-randomly, one read in 16 with an ID the header does not list), and one more JSON
line gives the UNGROUPED conversion of those bytes (bam_frame, bam_fastq) beside the grouped one (bam_groups_frame,
bam_groups_fastq: one stream per group plus one for the reads of no group), the emit launch's workgroups and the workspace
(vk_bam_groups_workspace_size).  Run from a tree whose library lacks the grouped calls (an older revision: tools/build_rev.sh,
VKIMG_LIB) the line holds the ungrouped figures only: the same bytes, the other build.

usage: python tools/bam_time.py [--reads N] [--len L] [--long-reads N] [--long-len L] [--reps R] [--groups N[,N...]]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADER_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n"


def group_ids(groups):
    return [b"run1_sup@v5_bc%04d" % g for g in range(groups)]


def make_bam(n, L, seed=1, groups=0):
    """The inflated bytes of an unaligned BAM of n reads of L bases: fixed-size records, names `rNNNNNNNN`.  groups: that
    many @RG lines, and every record ends in `RG:Z:run1_sup@v5_bcNNNN` (one in 16: NNNN = 9999, no listed group)."""
    rng = np.random.default_rng(seed)
    name_len = 10   # with its NUL
    aux = 3 + len(group_ids(1)[0]) + 1 if groups else 0
    body = 32 + name_len + (L + 1) // 2 + L + aux
    rec = np.zeros((n, 4 + body), dtype=np.uint8)
    fixed = struct.pack("<iiiBBHHHIiii", body, -1, -1, name_len, 0, 4680, 0, 4, L, -1, -1, 0)
    rec[:, :36] = np.frombuffer(fixed, dtype=np.uint8)
    rec[:, 36] = ord("r")
    idx = np.arange(n)
    for d in range(8):
        rec[:, 37 + d] = ord("0") + (idx // 10 ** (7 - d)) % 10
    codes = np.array([1, 2, 4, 8], dtype=np.uint8)[rng.integers(0, 4, (n, 2 * ((L + 1) // 2)), dtype=np.uint8)]
    if L % 2:
        codes[:, -1] = 0
    at = 36 + name_len
    rec[:, at:at + (L + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    rec[:, at + (L + 1) // 2:at + (L + 1) // 2 + L] = rng.integers(2, 41, (n, L), dtype=np.uint8)
    text = HEADER_TEXT
    if groups:
        which = rng.integers(0, groups, n)
        which[rng.integers(0, 16, n) == 0] = 9999
        tail = np.zeros((n, aux), dtype=np.uint8)
        tail[:, :aux - 1] = np.frombuffer(b"RGZ" + group_ids(1)[0], dtype=np.uint8)
        for d in range(4):
            tail[:, aux - 5 + d] = ord("0") + (which // 10 ** (3 - d)) % 10
        rec[:, 4 + body - aux:] = tail
        text += b"".join(b"@RG\tID:" + i + b"\tSM:s\n" for i in group_ids(groups))
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
    return np.concatenate([np.frombuffer(head, dtype=np.uint8), rec.ravel()]), len(head)


def bgzf(data, threads=16, member=0xFF00):
    def one(at):
        chunk = data[at:at + member].tobytes()
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = c.compress(chunk) + c.flush()
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    with ThreadPoolExecutor(threads) as pool:
        parts = list(pool.map(one, range(0, len(data), member)))
    eof = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0"
    return b"".join(parts) + eof


def best_of(fn, reps):
    fn()   # warm-up: workspaces are grown here
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return min(times), out


def measure(eng, n, L, reps, tmp):
    import torch
    from varkoder_amd import _capi, bam
    data, first = make_bam(n, L)
    path = os.path.join(tmp, f"reads_{n}x{L}.bam")
    with open(path, "wb") as f:
        f.write(bgzf(data))
    assert bam.bam_header(path)[:2] == (first, 0)
    timings = {}
    torch.cuda.synchronize()
    t = time.perf_counter()
    dev, offs, lens = eng.upload_staged(eng.stage_files([path]), timings)
    torch.cuda.synchronize()
    t_upload = time.perf_counter() - t
    assert int(lens[0]) == len(data)
    args = (dev, offs, lens, [first], [0], [0], [_capi.VK_BAM_ALL])
    row = {"reads": n, "read_len": L, "bam_bytes": os.path.getsize(path), "inflated_bytes": len(data),
           "upload_s": t_upload, "inflate_s": timings.get("inflate_s")}
    for tag, flags in (("", 0), ("_no_guess", _capi.VK_BAM_NO_GUESS)):
        t_frame, (recs, nbytes, status) = best_of(lambda: eng.bam_frame(*args, flags=flags), reps)
        assert not status.any() and int(recs[0]) == n and int(nbytes[0]) == n * (10 + 2 * L + 5)
        out = torch.zeros(int(nbytes[0]) + 32, dtype=torch.uint8, device=eng.device)
        t_fastq, (got, status) = best_of(lambda: eng.bam_fastq(*args, out, [0], nbytes, flags=flags), reps)
        segments, rewalked = eng.last_bam_frame()
        assert not status.any() and int(got[0]) == int(nbytes[0])
        row.update({f"frame_s{tag}": t_frame, f"fastq_s{tag}": t_fastq, f"emit_s{tag}": t_fastq - t_frame,
                    f"segments{tag}": segments, f"rewalked{tag}": rewalked})
    row["fastq_bytes"] = int(nbytes[0])
    row["fastq_gb_s"] = int(nbytes[0]) / row["fastq_s"] / 1e9
    del dev
    toffs, tlens = np.zeros(1, dtype=np.uint64), nbytes

    def clean():
        lines = eng.clean_lines(out, toffs, tlens)
        return eng.clean(out, toffs, tlens, lines // 4, [_capi.VK_CL_ROLE_UNPAIRED], [0], 1)
    t_clean, res = best_of(clean, reps)
    assert not res[4].any()
    row["clean_s"] = t_clean
    row["convert_over_clean"] = row["fastq_s"] / t_clean
    return row


def measure_groups(eng, n, L, groups, reps, tmp):
    """The ungrouped and the grouped conversion of one file of `groups` read groups."""
    import torch
    from varkoder_amd import _capi, bam
    data, first = make_bam(n, L, groups=groups)
    path = os.path.join(tmp, f"reads_{n}x{L}_g{groups}.bam")
    with open(path, "wb") as f:
        f.write(bgzf(data))
    assert bam.bam_header(path)[:2] == (first, 0)
    dev, offs, lens = eng.upload_staged(eng.stage_files([path]), {})
    args = (dev, offs, lens, [first], [0])
    row = {"reads": n, "read_len": L, "groups": groups, "inflated_bytes": len(data)}
    plain = args + ([0], [_capi.VK_BAM_ALL])
    t_frame, (recs, nbytes, status) = best_of(lambda: eng.bam_frame(*plain), reps)
    assert not status.any() and int(recs[0]) == n
    out = torch.zeros(int(nbytes[0]) + 32, dtype=torch.uint8, device=eng.device)
    t_fastq, _ = best_of(lambda: eng.bam_fastq(*plain, out, [0], nbytes), reps)
    row.update({"frame_s": t_frame, "fastq_s": t_fastq, "fastq_bytes": int(nbytes[0])})
    del out
    if not hasattr(eng, "bam_groups_frame"):   # (an older build: the ungrouped figures of the same bytes)
        return row
    ids = bam.read_groups(path)
    assert ids == group_ids(groups)
    sgroup = list(range(groups)) + [_capi.VK_BAM_UNGROUPED]
    grouped = args + ([ids], [0] * len(sgroup), [_capi.VK_BAM_ALL] * len(sgroup), sgroup)
    t_gframe, (grecs, gbytes, status) = best_of(lambda: eng.bam_groups_frame(*grouped), reps)
    assert not status.any() and int(grecs.sum()) == n and int(gbytes.sum()) == int(nbytes[0])
    oo = np.zeros(len(sgroup), dtype=np.uint64)
    oo[1:] = np.cumsum((gbytes[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))
    out = torch.zeros(int(oo[-1] + gbytes[-1]) + 32, dtype=torch.uint8, device=eng.device)
    t_gfastq, (got, status) = best_of(lambda: eng.bam_groups_fastq(*grouped, out, oo, gbytes), reps)
    assert not status.any() and np.array_equal(got, gbytes)
    wgs, walked = eng.last_bam_groups()
    row.update({"groups_frame_s": t_gframe, "groups_fastq_s": t_gfastq, "groups_emit_s": t_gfastq - t_gframe,
                "emit_workgroups": wgs, "aux_walked": walked, "ungrouped_reads": int(grecs[-1]),
                "workspace_bytes": eng.bam_groups_workspace_size(lens, [ids], [0] * len(sgroup)),
                "grouped_over_ungrouped": t_gfastq / t_fastq})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--long-reads", type=int, default=10_000)
    ap.add_argument("--long-len", type=int, default=15_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=lambda t: [int(x) for x in t.split(",")], default=[],
                    help="read groups of the short-read file, e.g. 1,96,1024: the grouped conversion beside the ungrouped one")
    a = ap.parse_args()
    from varkoder_amd.engine import ImageEngine
    eng = ImageEngine(k=7, mapping="cgr", device=0)
    with tempfile.TemporaryDirectory(prefix="bam_time_") as tmp:
        for n, L in ((a.reads, a.len), (a.long_reads, a.long_len)):
            if n and not a.groups:
                print(json.dumps(measure(eng, n, L, a.reps, tmp)), flush=True)
        for g in a.groups:
            print(json.dumps(measure_groups(eng, a.reads, a.len, g, a.reps, tmp)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
