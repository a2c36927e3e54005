"""Raw-read input of `image --from-raw` and `query --from-raw` (step B's host half): which files make a sample, how
they pair up and how many records of each the cleaning takes.  Behaviour of the reference's process_input
(core/utils.py:283-411), clean_reads' R1/R2 split (commands/image.py:358-384) and calculate_reads_needed (:164-221),
pinned on the reference's own functions by tests/golden/raw_input_cases.json and, for process_input's query branch,
tests/golden/query_input_cases.json."""
import re
from pathlib import Path

from .config import LABELS_SEP

RE_R1 = re.compile(r"(?<=[_R.])1(?=[_.])")
RE_R2 = re.compile(r"(?<=[_R.])2(?=[_.])")
FASTQ_SUFFIXES = ("fq", "fastq", "fq.gz", "fastq.gz")


def is_fastq_file(name):
    return str(name).endswith(FASTQ_SUFFIXES)


def process_input(inpath, is_query=False):
    """[(sample, labels, files)] sorted by sample: from a folder `<taxon>/<sample>/<reads>` (labels: the taxon
    folders the sample appears under) or from a CSV with columns labels, sample, files (';'-separated, files
    relative to the CSV's folder).  Labels and files are sorted and unique.

    is_query (core/utils.py:340-383): the input is a folder of reads to identify, labelled ["query"].  Without
    sub-folders every FASTQ file is a sample of its own, named by what precedes the first '.' of its file name
    (`s_1.fq` and `s_2.fq` are two samples; files whose names agree up to there are one).  With sub-folders (or links
    to folders) each of them is a sample made of the FASTQ files directly inside it, and files beside them are ignored."""
    inpath = Path(inpath)
    rows = []
    if is_query:
        import os
        entries = list(inpath.iterdir())
        if not any(f.is_dir() or (f.is_symlink() and Path(os.readlink(f)).is_dir()) for f in entries):
            for fl in inpath.rglob("*"):
                if is_fastq_file(fl.name):
                    rows.append((("query",), fl.name.split(".")[0], [str(fl)]))
        else:
            for sample in entries:
                if sample.resolve().is_dir():
                    for fl in sample.iterdir():
                        if is_fastq_file(fl.name):
                            rows.append((("query",), sample.name, [str(sample / fl.name)]))
        if not rows:   # (the reference fails here as well: pandas raises a KeyError ahead of its own check)
            raise Exception("Folder detected, but no records read. Check format.")
    elif inpath.is_dir():
        # (a sample under two taxa is one sample with both labels: the reference's duplicate check never fires)
        for taxon in inpath.iterdir():
            if not taxon.is_dir():
                continue
            for sample in taxon.iterdir():
                if not sample.is_dir():
                    continue
                for fl in sample.iterdir():
                    if is_fastq_file(fl.name):
                        rows.append(((taxon.name,), sample.name, [str(taxon / sample.name / fl.name)]))
        if not rows:
            raise Exception("Folder detected, but no records read. Check format.")
    else:
        import pandas as pd
        table = pd.read_csv(inpath)
        for col in ("labels", "sample", "files"):
            if col not in table.columns:
                raise Exception("Input csv file missing column: " + col)
        for _, r in table.iterrows():
            rows.append((tuple(str(r["labels"]).split(LABELS_SEP)), str(r["sample"]),
                         [str(Path(inpath.parent, z)) for z in str(r["files"]).split(";")]))
    merged = {}
    for labels, sample, files in rows:
        lab, fl = merged.setdefault(str(sample), (set(), set()))
        lab.update(labels)
        fl.update(files)
    return [(s, sorted(merged[s][0]), sorted(merged[s][1])) for s in sorted(merged)]


def pair_files(files):
    """{"R1": [...], "R2": [...], "unpaired": [...]}: a name whose `1` / `2` follows `_`, `R` or `.` and precedes `_`
    or `.` is R1 / R2; one without its mate goes to unpaired.  As in the reference, the check walks each list while
    it removes from it, so the file right after a mateless one is not looked at (kept on purpose: SURVEY Appendix A)."""
    files = [str(f) for f in files]
    r1 = [f for f in files if RE_R1.search(f)]
    r2 = [f for f in files if RE_R2.search(f)]
    unpaired = [f for f in files if f not in r1 + r2]
    for mine, pat, mate in ((r1, RE_R1, "2"), (r2, RE_R2, "1")):
        others = r2 if mine is r1 else r1
        i = 0
        while i < len(mine):
            f = mine[i]
            if pat.sub(mate, f) not in others:
                unpaired.append(f)
                del mine[i]
            i += 1     # (the element that moved into slot i is skipped)
    return {"R1": r1, "R2": r2, "unpaired": unpaired}


def avg_read_length(text, sample_size=10000):
    """Mean length of the (whitespace-stripped) sequence lines of the first `sample_size` records of FASTQ text."""
    total = n = 0
    for i, line in enumerate(text.split(b"\n")):
        if i % 4 == 1:
            total += len(line.strip())
            n += 1
            if n >= sample_size:
                break
    return total / n if n else 0


def reads_needed(files_info, max_bp):
    """{file: records to take}.  files_info = {"unpaired" | "R1" | "R2": [{"file", "avg_length", "total_reads"}]},
    each list sorted by file name.  max_bp None: everything (a pair: the shorter file's count); otherwise 5 x max_bp
    bases, single-end files first, then pairs; a file that gets no entry is not read."""
    take = {}
    if max_bp is None:
        for fi in files_info["unpaired"]:
            take[fi["file"]] = fi["total_reads"]
        for a, b in zip(files_info["R1"], files_info["R2"]):
            n = min(a["total_reads"], b["total_reads"])
            take[a["file"]] = take[b["file"]] = n
        return take
    remaining = 5 * max_bp
    for fi in files_info["unpaired"]:
        n = min(fi["total_reads"], int(remaining / fi["avg_length"]))
        take[fi["file"]] = n
        remaining -= n * fi["avg_length"]
    if remaining > 0:
        for a, b in zip(files_info["R1"], files_info["R2"]):
            per_pair = a["avg_length"] + b["avg_length"]
            n = min(min(a["total_reads"], b["total_reads"]), int(remaining / per_pair))
            take[a["file"]] = take[b["file"]] = n
            remaining -= n * per_pair
    return take


def content_curves(base, reach):
    """fastp-style content_curves {A, T, C, G: per-cycle fractions} from per-cycle base counts base[40][4] (A C G T)
    and the reads that reach each cycle; cycles no read reaches are left out."""
    import numpy as np
    base = np.asarray(base, dtype=np.float64).reshape(-1, 4)
    reach = np.asarray(reach, dtype=np.float64)
    n = int(np.count_nonzero(reach))
    frac = base[:n] / reach[:n, None]
    return {b: frac[:, "ACGT".index(b)].tolist() for b in "ATCG"}


def curves_sd(curves):
    """get_basefrequency_sd's figure for one set of curves: the std of each base's fraction over cycles 5..39,
    averaged over the four bases (nan when no read reaches cycle 5)."""
    import numpy as np
    rows = np.array([curves[b] for b in "ATCG"], dtype=np.float64)
    if rows.shape[1] <= 5:
        return float("nan")
    return float(np.std(rows[:, 5:40], axis=1).mean())
