"""`--kmer-spectrum`: what a k-mer spectrum row (ImageEngine.spectrum, include/vkimg.h VK_SPEC_*) says about a library --
k-mer and base coverage, the genome's distinct k-mers, the error rate, the share of high-copy k-mers -- and the files and
stats.csv columns that state it.  The rule and its limits: INTEGRATION.md, "`--kmer-spectrum`: the rule".  Pure Python
and NumPy: everything here works from a row alone."""
import json
import math
from pathlib import Path

import numpy as np

from . import _capi

NSTAT, HIST_AT, BINS = _capi.VK_SPEC_NSTAT, _capi.VK_SPEC_HIST, 256
READS, BASES, WINDOWS, TAKEN_WINDOWS, DISTINCT = range(5)
MIN_SUPPORT = 1000
ESTIMATES = ("kmer_coverage", "base_coverage", "genome_kmers", "error_kmers", "error_rate", "high_copy_fraction")
COLUMNS = ("kmer_coverage", "base_coverage", "genome_kmers", "error_rate", "high_copy_fraction")
K_DEFAULT, EVERY_DEFAULT = 21, 1


def estimate(row, k, every=1):
    """The estimates of a row counted at k with key sampling `every`: a dict of ESTIMATES, `singleton_fraction`,
    `support` and `reason`.  With h(c) the distinct k-mers of multiplicity c: c* is the smallest c in 2..254 that
    maximises h(c) + h(c + 1) (their sum is `support`), lambda = (c* + 1) h(c* + 1) / h(c*) -- the ratio a Poisson
    spectrum has at every c, taken where the most counts stand behind it, above the error singletons.  Every value of
    ESTIMATES is None, with a `reason`, when the spectrum does not carry them."""
    row = np.asarray(row, dtype=np.uint64)
    h = np.concatenate(([0], row[HIST_AT:HIST_AT + BINS].astype(np.int64)))   # h[c], c = 1..256 (256: that and more)
    W, distinct, bases = int(row[TAKEN_WINDOWS]), int(row[DISTINCT]), int(row[BASES])
    out = {name: None for name in ESTIMATES}
    out["singleton_fraction"] = int(h[1]) / distinct if distinct else None
    pair = h[2:255] + h[3:256]
    cstar = 2 + int(np.argmax(pair))   # (the first of equal maxima)
    out["support"], out["reason"] = int(pair[cstar - 2]), None
    if out["support"] < MIN_SUPPORT or h[cstar] == 0 or h[cstar + 1] == 0:
        out["reason"] = "too few repeated k-mers"
        return out
    if cstar == 254 and h[255] + h[256] > h[254]:
        out["reason"] = "coverage above the histogram"
        return out
    lam = (cstar + 1) * int(h[cstar + 1]) / int(h[cstar])
    genome = every * (distinct - int(h[1])) / (1.0 - math.exp(-lam) * (1.0 + lam))
    errors = max(int(h[1]) - (genome / every) * lam * math.exp(-lam), 0.0)
    top = min(256, max(8, math.ceil(4 * lam)))
    below = int((np.arange(1, top) * h[1:top]).sum())
    out.update(kmer_coverage=lam, base_coverage=bases / genome, genome_kmers=genome, error_kmers=errors,
               error_rate=1.0 - (1.0 - errors / W) ** (1.0 / k), high_copy_fraction=(W - below) / W)
    return out


def assembly_estimate(row, k, every=1):
    """The estimates of an assembly's row (ImageEngine.spectrum_fasta; the rule: INTEGRATION.md, "`--genome-spectrum`: the
    rule"): an assembly shows every k-mer of its genome once per copy, so genome_kmers = every x distinct,
    high_copy_fraction is the share of taken windows whose k-mer occurs more than once, seen_fraction is 1, and what
    describes a library (coverage, errors) is None."""
    row = np.asarray(row, dtype=np.uint64)
    taken, distinct, ones = int(row[TAKEN_WINDOWS]), int(row[DISTINCT]), int(row[HIST_AT])
    out = {name: None for name in ESTIMATES}
    out.update(genome_kmers=int(every) * distinct, high_copy_fraction=(taken - ones) / taken if taken else None,
               singleton_fraction=ones / distinct if distinct else None, seen_fraction=1.0, reason="assembly")
    return out


def report(row, k, every=1, sketch=None, assembly=False):
    """The object of `<sample>.spectrum.json`.  sketch (`--spectrum-sketch`: sketch.meta) becomes its `"sketch"` object;
    without one the object has no such key.  assembly (`--genome-spectrum`): the row counts records where a library's
    counts reads, the estimates are assembly_estimate's and the object says `"source": "assembly"`."""
    row = np.asarray(row, dtype=np.uint64)
    hist = [int(x) for x in row[HIST_AT:HIST_AT + BINS - 1]]
    while hist and hist[-1] == 0:
        hist.pop()
    out = {"k": int(k), "every": int(every), "records" if assembly else "reads": int(row[READS]), "bases": int(row[BASES]),
           "windows": int(row[WINDOWS]), "taken_windows": int(row[TAKEN_WINDOWS]), "distinct": int(row[DISTINCT]),
           "histogram": hist, "histogram_256_and_more": int(row[HIST_AT + BINS - 1]),
           "estimates": assembly_estimate(row, k, every) if assembly else estimate(row, k, every)}
    if assembly:
        out = {"source": "assembly", **out}
    if sketch is not None:
        out["sketch"] = dict(sketch)
    return out


ASSEMBLY_COLUMNS = ("genome_kmers", "high_copy_fraction")


def assembly_columns(row, k, every=1):
    """The stats.csv columns of an assembly's row: the spectrum_* cells that describe a library stay empty."""
    est = assembly_estimate(row, k, every)
    return {"spectrum_" + name: (est[name] if name in ASSEMBLY_COLUMNS and est[name] is not None else "") for name in COLUMNS}


def columns(row, k, every=1):
    """The stats.csv columns of a row: an estimate the spectrum does not carry gives an empty cell."""
    est = estimate(row, k, every)
    return {"spectrum_" + name: ("" if est[name] is None else est[name]) for name in COLUMNS}


def report_path(folder, sample):
    return Path(folder) / (sample + ".spectrum.json")


def write_report(folder, sample, obj):
    path = report_path(folder, sample)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as fh:
        json.dump(obj, fh)
