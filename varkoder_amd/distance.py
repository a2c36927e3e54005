"""`distance`: genomic distances between samples from their k-mers.  Neither the reference nor any other command here
compares samples by their k-mers; the rule is this project's ("`--spectrum-sketch` and `distance`: the
rule").

The samples are the `<sample>.spectrum.json` files of a folder that carry a `"sketch"` object, each with its
`<sample>.sketch.npy` (`image / query --kmer-spectrum DIR --spectrum-sketch S` for reads, `--from-fasta --genome-spectrum DIR
--spectrum-sketch S` for assemblies).  One call (ImageEngine.sketch_pairs:
vk_sketch_pairs_device, csrc/vk_sketch.h) compares every query sketch with every reference sketch; the distances
(sketch.py) and the ranking are computed on the host from its integers.  There is no CPU path for the comparison.

Outputs in OUT: distances.csv (a row per sample and rank), with --matrix shared.npy, seen.npy, corrected_distance.npy and
the names of their rows and columns.
"""
import json
from pathlib import Path

import numpy as np

from . import sketch
from .image import eprint

COLUMNS = ["sample", "neighbour", "rank", "shared", "seen", "jaccard", "mash_distance", "corrected_distance"]
SUFFIX = ".spectrum.json"
SAME = ("k", "every") + sketch.META_KEYS


class SketchSet:
    """The sketched samples of a folder: names, reports (the json objects), rows uint64[n, size] and lengths."""

    def __init__(self, folder):
        self.folder = Path(folder)
        self.names, self.reports, self.paths, hashes = [], [], [], []
        for path in sorted(self.folder.glob("*" + SUFFIX)):
            with open(path) as fh:
                rep = json.load(fh)
            if "sketch" not in rep:
                continue
            name = path.name[:-len(SUFFIX)]
            h = np.load(sketch.sketch_path(self.folder, name))
            sk = rep["sketch"]
            if h.dtype != np.uint64 or h.ndim != 1 or len(h) != sk["length"] or len(h) > sk["size"]:
                raise Exception(f"{sketch.sketch_path(self.folder, name)}: not the sketch that {path} describes")
            self.names.append(name)
            self.reports.append(rep)
            self.paths.append(path)
            hashes.append(h)
        if not self.names:
            raise Exception(f"{self.folder}: no {SUFFIX} file with a sketch (made with --kmer-spectrum DIR --spectrum-sketch S)")
        self.size = int(self.reports[0]["sketch"]["size"])
        self.lengths = np.array([len(h) for h in hashes], dtype=np.uint64)
        self.rows = np.full((len(hashes), self.size), np.uint64(2 ** 64 - 1), dtype=np.uint64)
        for i, h in enumerate(hashes):
            self.rows[i, :min(len(h), self.size)] = h[:self.size]

    def signature(self, i):
        rep = self.reports[i]
        return tuple(rep[x] if x in ("k", "every") else rep["sketch"][x] for x in SAME)


def is_assembly(rep):
    """A report of `--genome-spectrum`: its sketch holds every k-mer of an assembly, whatever reads were thresholded at."""
    return rep.get("source") == "assembly"


def check_comparable(sets):
    """Sketches compare only when k, every, size, hash and version agree everywhere and min_count among the samples of
    reads (an assembly's report is exempt from that one): the first two files that differ are named."""
    at = SAME.index("min_count")
    first = (sets[0].paths[0], sets[0].signature(0))
    first_reads = None   # the first sample of reads: what min_count is held against
    for st in sets:
        for i, path in enumerate(st.paths):
            sig = st.signature(i)
            ref = first
            if not is_assembly(st.reports[i]):
                if first_reads is None:
                    first_reads = (path, sig)
                ref = first_reads
            pairs = [(name, a, b) for name, a, b in zip(SAME, first[1], sig) if name != "min_count" and a != b]
            if pairs:
                ref = first
            elif ref is first_reads and ref[1][at] != sig[at]:
                pairs = [("min_count", ref[1][at], sig[at])]
            if pairs:
                what = ", ".join(f"{name} {a} and {b}" for name, a, b in pairs)
                raise Exception(f"sketches that do not compare: {ref[0]} and {path} differ in {what}")
    if first[1][SAME.index("hash")] != sketch.HASH or first[1][SAME.index("version")] != sketch.VERSION:
        raise Exception(f"{first[0]}: a sketch of hash {first[1][SAME.index('hash')]!r}, version {first[1][SAME.index('version')]}; "
                        f"this program compares {sketch.HASH!r}, version {sketch.VERSION}")


def pair_values(q, r, i, j, shared, seen):
    """(jaccard, mash_distance, corrected_distance) of query i and reference j."""
    a, b = q.reports[i], r.reports[j]
    jac = sketch.jaccard(int(shared[i, j]), int(seen[i, j]))
    eta1, g1 = sketch.sample_eta(a["estimates"], a["sketch"]["min_count"])
    eta2, g2 = sketch.sample_eta(b["estimates"], b["sketch"]["min_count"])
    return (jac, sketch.mash_distance(jac, a["k"]),
            sketch.corrected_distance_eta(jac, a["k"], a["every"], a["sketch"]["eligible"], g1, eta1, b["sketch"]["eligible"], g2,
                                          eta2))


def rank_neighbours(shared, seen, n, exclude_self):
    """Per query the references in order: jaccard descending (compared exactly, as fractions), then the lower index."""
    order = []
    for i in range(shared.shape[0]):
        sh, se = shared[i].astype(np.int64), seen[i].astype(np.int64)
        jac = np.where(se > 0, sh / np.maximum(se, 1), -1.0)   # (nothing seen: behind every other)
        idx = np.lexsort((np.arange(len(jac)), -jac))
        if exclude_self:
            idx = idx[idx != i]
        order.append([int(x) for x in idx[:n]])
    return order


def table(q, r, shared, seen, n, exclude_self):
    """distances.csv: a row per query and rank (from 1)."""
    import pandas as pd
    rows = []
    for i, near in enumerate(rank_neighbours(shared, seen, n, exclude_self)):
        for rank, j in enumerate(near):
            jac, mash, corr = pair_values(q, r, i, j, shared, seen)
            rows.append({"sample": q.names[i], "neighbour": r.names[j], "rank": rank + 1, "shared": int(shared[i, j]),
                         "seen": int(seen[i, j]), "jaccard": "" if jac is None else jac,
                         "mash_distance": "" if mash is None else mash, "corrected_distance": "" if corr is None else corr})
    return pd.DataFrame(rows, columns=COLUMNS)


def corrected_matrix(q, r, shared, seen):
    out = np.full(shared.shape, np.nan, dtype=np.float64)
    for i in range(shared.shape[0]):
        for j in range(shared.shape[1]):
            d = pair_values(q, r, i, j, shared, seen)[2]
            if d is not None:
                out[i, j] = d
    return out


def refuse_early(args):
    """What can be refused before anything is read or the GPU is touched."""
    from .shard import world_info
    if world_info()[1] > 1:
        raise Exception("distance runs on one GPU: start it without a launcher (WORLD_SIZE > 1 is refused; the comparison "
                        "is not sharded)")
    if args.against and not Path(args.against).exists():
        raise Exception("Input path", args.against, "does not exist. Please check.")
    if not args.overwrite and Path(args.outdir).exists():
        raise Exception("Output directory exists, use --overwrite if you want to overwrite it.")


def write_outputs(outdir, q, r, shared, seen, n, exclude_self, matrix):
    outdir = Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    df = table(q, r, shared, seen, n, exclude_self)
    df.to_csv(outdir / "distances.csv", index=False)
    if matrix:
        np.save(outdir / "shared.npy", shared)
        np.save(outdir / "seen.npy", seen)
        np.save(outdir / "corrected_distance.npy", corrected_matrix(q, r, shared, seen))
        (outdir / "distances_rows.txt").write_text("".join(f"{p}\n" for p in q.names))
        (outdir / "distances_cols.txt").write_text("".join(f"{p}\n" for p in r.names))
    return df


def run_distance(args, pairs=None):
    """The `distance` sub-command; returns distances.csv as written.  pairs (tests): a function (q rows, q lengths, r
    rows, r lengths, size) -> (shared, seen) in place of the engine's."""
    refuse_early(args)
    eprint("Starting distance command.")
    q = SketchSet(args.input)
    r = SketchSet(args.against) if args.against else q
    check_comparable([q, r] if args.against else [q])
    eprint(f"Comparing {len(q.names)} sketches with {len(r.names)}.")
    if pairs is not None:
        shared, seen = pairs(q.rows, q.lengths, r.rows, r.lengths, q.size)
    else:
        from .engine import ImageEngine
        from .shard import world_info
        eng = ImageEngine(k=7, mapping="cgr", device=world_info()[2])   # (k and mapping are not used)
        try:
            shared, seen = eng.sketch_pairs(q.rows, q.lengths, q.rows if r is q else r.rows, r.lengths, q.size)
        finally:
            eng.close()
    return write_outputs(args.outdir, q, r, shared, seen, args.neighbours, not args.against, args.matrix)
