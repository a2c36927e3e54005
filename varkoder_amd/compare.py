"""`compare`: which images of a collection look alike, without a model.  Neither the reference nor any other command
here compares images with each other; the rule is this project's ("`compare`: the rule").

The images are collected and read as `train` does (train.collect_images, train.image_set), stay in HBM as uint8
[n, side, side], and one call (ImageEngine.neighbours: vk_dist_device, csrc/vk_dist.h) gives every image its nearest
others by exact squared Euclidean distance, computed on the i8 matrix cores.  A varKode is a rank-quantile image, so
that distance grows with how differently two samples rank their k-mers.  There is no CPU path.

Outputs in OUT: neighbours.csv (a row per image and rank), samples.csv (a row per image: its nearest distance and
whether its neighbours carry its labels: the column that finds mislabels), with --matrix distances.npy and the paths
of its rows and columns.
"""
import math
from pathlib import Path

import numpy as np

from .config import LABELS_SEP
from .image import eprint

NO_IDX = 0xFFFFFFFF
MATRIX_MAX_BYTES = 4 << 30
NEIGHBOUR_COLUMNS = ["sample", "bp", "img_kmer_mapping", "img_kmer_size", "path", "labels", "rank", "neighbour_sample",
                     "neighbour_bp", "neighbour_path", "neighbour_labels", "sq_distance", "distance", "shared_labels"]
SAMPLE_COLUMNS = ["sample", "bp", "path", "labels", "nearest_distance", "majority_labels", "own_labels_in_majority"]


def label_set(text):
    return {x for x in str(text).split(LABELS_SEP) if x}


def distance(sq, npix):
    """The root-mean-square pixel difference as a share of the full range: a float64 from the exact integer."""
    return math.sqrt(int(sq) / npix) / 255


def groups_of(df, same_sample=False):
    """The group id of every image of a set compared with itself: the ordinal of its sample (an image is then no
    neighbour of itself nor of the other ladder steps of its sample), or with same_sample its own ordinal (only the image
    itself is excluded)."""
    if same_sample:
        return np.arange(len(df), dtype=np.uint32)
    ordinal = {}
    return np.array([ordinal.setdefault(s, len(ordinal)) for s in df["sample"]], dtype=np.uint32)


def neighbour_table(qdf, rdf, idx, d2, npix):
    """neighbours.csv: a row per query image and rank (from 1); fill slots produce no row."""
    import pandas as pd
    rows = []
    q, r = qdf.to_dict("records"), rdf.to_dict("records")
    for i, a in enumerate(q):
        for rank in range(idx.shape[1]):
            if int(idx[i, rank]) == NO_IDX:
                break
            b = r[int(idx[i, rank])]
            rows.append({"sample": a["sample"], "bp": a["bp"], "img_kmer_mapping": a["img_kmer_mapping"],
                         "img_kmer_size": a["img_kmer_size"], "path": str(a["path"]), "labels": a["labels"], "rank": rank + 1,
                         "neighbour_sample": b["sample"], "neighbour_bp": b["bp"], "neighbour_path": str(b["path"]),
                         "neighbour_labels": b["labels"], "sq_distance": int(d2[i, rank]), "distance": distance(d2[i, rank], npix),
                         "shared_labels": LABELS_SEP.join(sorted(label_set(a["labels"]) & label_set(b["labels"])))})
    return pd.DataFrame(rows, columns=NEIGHBOUR_COLUMNS)


def sample_table(qdf, rdf, idx, d2, npix):
    """samples.csv: a row per query image.  majority_labels: the labels more than half of its neighbours carry;
    own_labels_in_majority: the share of its own labels among those (empty for an image without labels)."""
    import pandas as pd
    rows = []
    rlabels = [label_set(x) for x in rdf["labels"]]
    for i, a in enumerate(qdf.to_dict("records")):
        near = [int(j) for j in idx[i] if int(j) != NO_IDX]
        counts = {}
        for j in near:
            for lab in rlabels[j]:
                counts[lab] = counts.get(lab, 0) + 1
        majority = sorted(lab for lab, c in counts.items() if 2 * c > len(near))
        own = label_set(a["labels"])
        rows.append({"sample": a["sample"], "bp": a["bp"], "path": str(a["path"]), "labels": a["labels"],
                     "nearest_distance": distance(d2[i, 0], npix) if near else "",
                     "majority_labels": LABELS_SEP.join(majority),
                     "own_labels_in_majority": len(own & set(majority)) / len(own) if own else ""})
    return pd.DataFrame(rows, columns=SAMPLE_COLUMNS)


def refuse_early(args):
    """What can be refused before anything is read or the GPU is touched."""
    from .shard import world_info
    if world_info()[1] > 1:
        raise Exception("compare runs on one GPU: start it without a launcher (WORLD_SIZE > 1 is refused; the comparison "
                        "is not sharded)")
    if args.against and not Path(args.against).exists():
        raise Exception("Input path", args.against, "does not exist. Please check.")
    if not args.overwrite and Path(args.outdir).exists():
        raise Exception("Output directory exists, use --overwrite if you want to overwrite it.")


def run_compare(args):
    """The `compare` sub-command; returns (neighbours, samples) as written."""
    from .engine import ImageEngine
    from .shard import world_info
    from .train import collect_images, image_set
    refuse_early(args)
    eprint("Starting compare command.")
    qdf = collect_images(args.input, args.label_table, args.verbose).reset_index(drop=True)
    rdf = collect_images(args.against, args.label_table, args.verbose).reset_index(drop=True) if args.against else qdf
    if args.matrix and 8 * len(qdf) * len(rdf) > MATRIX_MAX_BYTES:
        raise Exception(f"--matrix: {len(qdf)} x {len(rdf)} distances are more than 4 GiB; compare without it.")
    device = world_info()[2]
    eng = ImageEngine(k=7, mapping="cgr", device=device)   # (k and mapping are not used: the images exist)
    try:
        # one set, so that sizes that differ between IMAGES and REF_IMAGES are refused as mixed sizes within one are
        paths = list(qdf["path"]) + (list(rdf["path"]) if args.against else [])
        images = image_set(paths, eng if getattr(args, "gpu_png_read", False) else None).to(eng.device)
        q = images[:len(qdf)]
        r = images[len(qdf):] if args.against else q
        npix = int(images.shape[1]) * int(images.shape[2])
        groups = None if args.against else groups_of(qdf, args.same_sample)
        eprint(f"Comparing {len(qdf)} images with {len(rdf)}.")
        got = eng.neighbours(q, r, n=args.neighbours, qgroup=groups, rgroup=groups, matrix=args.matrix)
        idx, d2 = got[0], got[1]
        outdir = Path(args.outdir)
        outdir.mkdir(parents=True, exist_ok=True)
        neighbours, samples = neighbour_table(qdf, rdf, idx, d2, npix), sample_table(qdf, rdf, idx, d2, npix)
        neighbours.to_csv(outdir / "neighbours.csv", index=False)
        samples.to_csv(outdir / "samples.csv", index=False)
        if args.matrix:
            np.save(outdir / "distances.npy", got[2].cpu().numpy().view(np.uint64))
            (outdir / "distances_rows.txt").write_text("".join(f"{p}\n" for p in qdf["path"]))
            (outdir / "distances_cols.txt").write_text("".join(f"{p}\n" for p in rdf["path"]))
        return neighbours, samples
    finally:
        eng.close()
