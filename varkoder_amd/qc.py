"""`--qc-report`: the report and the stats.csv columns made of the rows that ImageEngine.qc counts on the GPU
(vk_qc_device; the rule: INTEGRATION.md, "--qc-report: the rule").  Host arithmetic on a few kilobytes per sample; the
key names are fastp's wherever the meaning is the same (the reference copies fastp's reports next to the cleaned reads,
commands/image.py:545-547)."""
import json
from pathlib import Path

import numpy as np

from . import _capi

NSTAT = _capi.VK_QC_NSTAT
CYCLES, PHREDS, LEN_BINS, CLASSES = _capi.VK_QC_CYCLES, 94, 1025, 5
RECORDS, RAGGED, BASES, GC, OTHER, MIN_LEN, MAX_LEN, INVALID = range(8)
QUAL_AT, READQ_AT, LEN_AT = _capi.VK_QC_QUAL_HIST, _capi.VK_QC_READQ_HIST, _capi.VK_QC_LEN_HIST
BASE_AT, QSUM_AT = _capi.VK_QC_CYCLE_BASE, _capi.VK_QC_CYCLE_QSUM
ROLE_KEYS = ("single", "read1", "read2")   # by _capi.VK_CL_ROLE_UNPAIRED, _R1, _R2


def counted(row):
    """The records of a row that were counted: all but the ragged ones."""
    return int(row[RECORDS]) - int(row[RAGGED])


def add_rows(rows):
    """The row of several streams taken together: every counter summed, min_length and max_length the smallest and the
    largest over the rows that counted a record (0 without one).  No rows: the zero row."""
    out = np.zeros(NSTAT, dtype=np.uint64)
    lo, hi = [], []
    for r in rows:
        r = np.asarray(r, dtype=np.uint64)
        out += r
        if counted(r):
            lo.append(int(r[MIN_LEN]))
            hi.append(int(r[MAX_LEN]))
    out[MIN_LEN], out[MAX_LEN] = (min(lo), max(hi)) if lo else (0, 0)
    return out


def _rate(a, b):
    return float(a) / float(b) if b else 0.0


def totals(row):
    """fastp's summary figures of a row.  total_reads counts every record, the ragged ones too; mean_length is over the
    counted ones."""
    qual = row[QUAL_AT:QUAL_AT + PHREDS]
    bases, q20, q30 = int(row[BASES]), int(qual[20:].sum()), int(qual[30:].sum())
    return {"total_reads": int(row[RECORDS]), "total_bases": bases, "q20_bases": q20, "q30_bases": q30,
            "q20_rate": _rate(q20, bases), "q30_rate": _rate(q30, bases), "mean_length": _rate(bases, counted(row)),
            "gc_content": _rate(int(row[GC]), bases)}


def profile(row):
    """A section of the report (`read1_before_filtering`, ..., `after_filtering`) for a row."""
    row = np.asarray(row, dtype=np.uint64)
    n = min(int(row[MAX_LEN]), CYCLES)
    base = row[BASE_AT:BASE_AT + CYCLES * CLASSES].reshape(CYCLES, CLASSES)[:n].astype(np.float64)
    qsum = row[QSUM_AT:QSUM_AT + CYCLES * CLASSES].reshape(CYCLES, CLASSES)[:n].astype(np.float64)
    reach = base.sum(axis=1)

    def over(a, b):   # a / b per cycle, 0.0 where nothing was counted
        return np.divide(a, b, out=np.zeros(n), where=b > 0).tolist()

    col = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    quality = {b: over(qsum[:, col[b]], base[:, col[b]]) for b in "ATCG"}
    quality["mean"] = over(qsum.sum(axis=1), reach)
    content = {b: over(base[:, col[b]], reach) for b in "ATCGN"}
    content["GC"] = over(base[:, 1] + base[:, 2], reach)
    out = totals(row)
    out.update({"total_cycles": n, "min_length": int(row[MIN_LEN]), "max_length": int(row[MAX_LEN]),
                "ragged_reads": int(row[RAGGED]), "invalid_quality_bytes": int(row[INVALID]),
                "quality_curves": quality, "content_curves": content,
                # length_histogram[l]: reads of l bases, up to the longest (its last bin, 1024, holds every longer read)
                "length_histogram": [int(v) for v in row[LEN_AT:LEN_AT + min(int(row[MAX_LEN]), LEN_BINS - 1) + 1]],
                "quality_histogram": [int(v) for v in row[QUAL_AT:QUAL_AT + PHREDS]],
                "read_mean_quality_histogram": [int(v) for v in row[READQ_AT:READQ_AT + PHREDS]]})
    return out


def report(before_by_role, after):
    """The object of `<sample>.qc.json`: before_by_role {"read1" | "read2" | "single": row} for the roles that have files
    (None or empty: a run that saw cleaned reads only -- the `after` sections alone), after: the cleaned text's row."""
    out = {"summary": {}}
    if before_by_role:
        out["summary"]["before_filtering"] = totals(add_rows(before_by_role.values()))
    out["summary"]["after_filtering"] = totals(np.asarray(after, dtype=np.uint64))
    for role in ("read1", "read2", "single"):
        if before_by_role and role in before_by_role:
            out[role + "_before_filtering"] = profile(before_by_role[role])
    out["after_filtering"] = profile(after)
    return out


def columns(before, after):
    """The stats.csv columns: before = the raw rows taken together (add_rows) or None, after = the cleaned text's row."""
    out = {}
    if before is not None:
        t = totals(np.asarray(before, dtype=np.uint64))
        out.update({"raw_reads": t["total_reads"], "raw_basepairs": t["total_bases"], "raw_q30_rate": t["q30_rate"]})
    t = totals(np.asarray(after, dtype=np.uint64))
    out.update({"clean_reads": t["total_reads"], "clean_q30_rate": t["q30_rate"], "clean_gc_content": t["gc_content"],
                "clean_mean_length": t["mean_length"]})
    return out


def report_path(folder, sample):
    """`<folder>/<sample>.qc.json` (not `*_fastp_*.json`: image.base_sd_table globs those)."""
    return Path(folder) / (sample + ".qc.json")


def write_report(folder, sample, obj):
    path = report_path(folder, sample)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as fh:
        json.dump(obj, fh)
