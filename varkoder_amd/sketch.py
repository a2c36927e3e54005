"""`--spectrum-sketch` and `distance`: what two samples' bottom-s sketches (ImageEngine.spectrum(sketch=...),
ImageEngine.sketch_pairs) say about the distance between their genomes, and the files that carry a sketch.  The rule, its
derivation and its limits: INTEGRATION.md, "`--spectrum-sketch` and `distance`: the rule".  Pure Python: everything here
works from the pair's integers and the spectrum's estimates alone."""
import math
from pathlib import Path

import numpy as np

HASH, VERSION = "splitmix64-finaliser", 1
META_KEYS = ("size", "min_count", "hash", "version")   # what two sketches must share, beside the spectrum's k and every


def jaccard(shared, seen):
    """shared / seen; None when nothing was seen (two empty sketches)."""
    return None if seen == 0 else shared / seen


def mash_distance(j, k):
    """-(1/k) ln(2J / (1 + J)): the Mash distance of a raw Jaccard index; 1.0 when J = 0, None when J is."""
    if j is None:
        return None
    return 1.0 if j <= 0 else max(0.0, -math.log(2.0 * j / (1.0 + j)) / k)


def seen_fraction(lam, m):
    """eta = P(Poisson(lam) >= m): the share of a genome's k-mers that a library of k-mer coverage lam shows m times or more."""
    term, below = math.exp(-lam), 0.0
    for c in range(m):
        below += term
        term *= lam / (c + 1)
    return max(0.0, 1.0 - below)


def corrected_distance(j, k, every, m, a1, est1, a2, est2):
    """The distance between the genomes behind two samples, corrected for their depths.  a_i: sample i's eligible count
    (measured: error k-mers are in it); est_i: its spectrum estimates (spectrum.estimate: kmer_coverage lambda_i,
    genome_kmers G_i).  The observed intersection is I = J (a1 + a2) / (1 + J); a k-mer of both genomes is seen in both
    samples with probability eta_1 eta_2 and taken with probability 1 / every, so (1 - D)^k = 2 every I / (eta_1 eta_2 (G_1
    + G_2)) and D = 1 - min(1, that)^(1/k).  None when J is, or when either sample's estimates are."""
    if j is None or est1 is None or est2 is None:
        return None
    lam1, g1, lam2, g2 = est1.get("kmer_coverage"), est1.get("genome_kmers"), est2.get("kmer_coverage"), est2.get("genome_kmers")
    if lam1 is None or g1 is None or lam2 is None or g2 is None:
        return None
    return corrected_distance_eta(j, k, every, a1, g1, seen_fraction(lam1, m), a2, g2, seen_fraction(lam2, m))


def corrected_distance_eta(j, k, every, a1, g1, eta1, a2, g2, eta2):
    """corrected_distance in its per-sample form: sample i shows a share eta_i of its genome's G_i k-mers (sample_eta).
    Two assemblies (eta = 1, G = every a) give D = 1 - (2J / (1 + J))^(1/k), the Mash distance's exact form.  None when J or
    any of a sample's two values is."""
    if j is None or g1 is None or g2 is None or eta1 is None or eta2 is None:
        return None
    eta = eta1 * eta2
    if eta <= 0.0 or g1 + g2 <= 0.0:
        return None
    inter = j * (a1 + a2) / (1.0 + j)
    x = 2.0 * every * inter / (eta * (g1 + g2))
    return 1.0 - min(1.0, x) ** (1.0 / k)


def _map(fn, x):
    """fn over the distinct values of a float64 array: the scalar function itself decides every value, so an array
    function built on it cannot differ from it in a last bit (NumPy's own log and power may, from one build to the next)."""
    uniq, inv = np.unique(x, return_inverse=True)
    return np.array([fn(float(v)) for v in uniq], dtype=np.float64)[inv.reshape(x.shape)]


def jaccard_np(shared, seen):
    """jaccard over integer arrays: float64, NaN where nothing was seen."""
    shared, seen = np.asarray(shared, dtype=np.float64), np.asarray(seen, dtype=np.float64)
    return np.where(seen > 0, shared / np.where(seen > 0, seen, 1.0), np.nan)


def mash_distance_np(shared, seen, k):
    """mash_distance(jaccard(shared, seen), k) of every entry, exactly: float64, NaN where it is None."""
    j = jaccard_np(shared, seen)
    ok = ~np.isnan(j)
    pos = ok & (j > 0)
    ratio = np.where(pos, 2.0 * j / (1.0 + j), 1.0)
    d = -_map(math.log, ratio) / k
    d = np.where(d > 0.0, d, 0.0)   # (max(0.0, d) as Python takes it: +0.0 unless d is greater)
    return np.where(pos, d, np.where(ok, 1.0, np.nan))


def corrected_distance_np(shared, seen, k, every, a, g, eta):
    """corrected_distance_eta of every pair of a square comparison, exactly: shared and seen integer arrays [n, n] (or
    [r, n, n]); a (eligible counts), g (genome_kmers) and eta per sample [n], NaN where a sample has none.  float64, NaN
    where the scalar function gives None."""
    j = jaccard_np(shared, seen)
    a = np.asarray(a, dtype=np.float64)
    g = np.array([np.nan if v is None else v for v in g], dtype=np.float64)
    eta = np.array([np.nan if v is None else v for v in eta], dtype=np.float64)
    e2 = eta[:, None] * eta[None, :]
    g2 = g[:, None] + g[None, :]
    a2 = a[:, None] + a[None, :]
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(j) & ~np.isnan(e2) & ~np.isnan(g2) & (e2 > 0.0) & (g2 > 0.0)
    jj = np.where(ok, j, 0.0)
    inter = jj * a2 / (1.0 + jj)
    x = 2.0 * every * inter / np.where(ok, e2 * g2, 1.0)
    root = 1.0 / k
    p = _map(lambda v: v ** root, np.where(ok, np.minimum(1.0, x), 1.0))
    return np.where(ok, 1.0 - p, np.nan)


def sample_eta(est, m):
    """(eta, G) of a sample from its spectrum estimates: eta is `seen_fraction` when the estimates state it (an assembly:
    1.0), else P(Poisson(kmer_coverage) >= m) with m the sample's own min_count; (None, None) without estimates."""
    if est is None or est.get("genome_kmers") is None:
        return None, None
    if est.get("seen_fraction") is not None:
        return float(est["seen_fraction"]), est["genome_kmers"]
    if est.get("kmer_coverage") is None:
        return None, None
    return seen_fraction(est["kmer_coverage"], m), est["genome_kmers"]


def meta(size, min_count, eligible, length):
    """The `"sketch"` object of `<sample>.spectrum.json`."""
    return {"size": int(size), "min_count": int(min_count), "eligible": int(eligible), "length": int(length), "hash": HASH,
            "version": VERSION}


def sketch_path(folder, sample):
    return Path(folder) / (sample + ".sketch.npy")


def write_sketch(folder, sample, hashes):
    """`<folder>/<sample>.sketch.npy`: the sketch's `length` hashes, u64, ascending."""
    path = sketch_path(folder, sample)
    path.parent.mkdir(parents=True, exist_ok=True)
    np.save(path, np.ascontiguousarray(hashes, dtype=np.uint64))
