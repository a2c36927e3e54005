#!/usr/bin/env python3
"""Golden cases for `image --from-raw`'s host half, made by running the reference's own process_input
(core/utils.py:283-411), clean_reads' R1/R2 split (commands/image.py:358-384) and calculate_reads_needed
(:164-221) unmodified.  Build-container only (needs the reference tree, imported through oracle/ref_harness.py).
clean_reads is driven with concatenate_reads replaced by a recorder that keeps its `reads` argument and raises,
so nothing past the split runs.  Writes tests/golden/raw_input_cases.json; varkoder_amd/rawinput.py must
reproduce every case (tests/test_clean_rules.py).

Usage:  python tools/gen_raw_input_golden.py
"""
import json
import shutil
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import ref_harness  # noqa: E402

ref_harness.install()
import varKoder.commands.image as ref_image  # noqa: E402
from varKoder.core.utils import process_input  # noqa: E402

# folder input: <taxon>/<sample>/<files>; one sample under two taxa, a non-FASTQ file, loose files at the top
TREE = {
    "taxonA/s1": ["s1_R1.fq.gz", "s1_R2.fq.gz", "s1_extra.fastq"],
    "taxonA/s2": ["s2.1.fq", "s2.2.fq", "notes.txt"],
    "taxonB/s3": ["lib_1.fastq.gz", "lib_2.fastq.gz", "other_1.fq"],
    "taxonC/s1": ["s1_more.fq"],
}
LOOSE = ["readme.fq"]

# file lists for the R1 / R2 split; the mateless R1 right after another mateless R1 stays in R1 (the reference
# deletes from the list it walks)
PAIRINGS = {
    "plain_pair": ["a_R1.fq", "a_R2.fq"],
    "dot_pair": ["a.1.fq.gz", "a.2.fq.gz"],
    "single_only": ["reads.fq"],
    "pair_and_single": ["x_1.fq", "x_2.fq", "x_single.fastq"],
    "mateless_r1": ["m_1.fq", "n_R1.fq"],
    "two_mateless_r1_in_a_row": ["a_1.fq", "b_1.fq", "c_1.fq", "c_2.fq"],
    "three_mateless_r1": ["p_1.fq", "q_1.fq", "r_1.fq"],
    "mateless_r2": ["u_2.fq", "v_1.fq", "v_2.fq"],
    "two_mateless_r2_in_a_row": ["g_2.fq", "h_2.fq", "i_2.fq"],
    "digit_not_delimited": ["s11.fq", "s12.fq", "R1x.fq"],
    "two_libraries": ["L1_R1_001.fastq.gz", "L1_R2_001.fastq.gz", "L2_R1_001.fastq.gz", "L2_R2_001.fastq.gz"],
}

BUDGETS = [
    ("everything", None, {"unpaired": [("u.fq", 150, 1000)], "R1": [("a_1.fq", 150, 800)], "R2": [("a_2.fq", 150, 700)]}),
    ("unpaired_enough", 10000, {"unpaired": [("u.fq", 100, 1000)], "R1": [("a_1.fq", 150, 800)], "R2": [("a_2.fq", 150, 800)]}),
    ("unpaired_then_pairs", 50000, {"unpaired": [("u.fq", 100, 1000)], "R1": [("a_1.fq", 150, 800)],
                                    "R2": [("a_2.fq", 149, 900)]}),
    ("pairs_only", 20000, {"unpaired": [], "R1": [("a_1.fq", 150, 1000), ("b_1.fq", 101, 50)],
                           "R2": [("a_2.fq", 150, 1000), ("b_2.fq", 99, 60)]}),
    ("more_r1_than_r2", None, {"unpaired": [], "R1": [("a_1.fq", 150, 10), ("b_1.fq", 150, 10)],
                               "R2": [("a_2.fq", 150, 12)]}),
    ("short_budget", 7, {"unpaired": [("u.fq", 3, 100)], "R1": [("a_1.fq", 2, 100)], "R2": [("a_2.fq", 2, 100)]}),
]


class Recorded(Exception):
    pass


def pairing(files):
    got = {}

    def record(reads, *a, **k):
        got.update({key: list(v) for key, v in reads.items()})
        raise Recorded()
    saved = ref_image.concatenate_reads
    ref_image.concatenate_reads = record
    tmp = tempfile.mkdtemp(prefix="pairing_")
    before = set(Path(tempfile.gettempdir()).glob("barcoding_clean_*"))
    try:
        ref_image.clean_reads(files, Path(tmp) / "out.fq.gz")
    except Recorded:
        pass
    finally:
        ref_image.concatenate_reads = saved
        shutil.rmtree(tmp)
        for d in set(Path(tempfile.gettempdir()).glob("barcoding_clean_*")) - before:
            shutil.rmtree(d, ignore_errors=True)
    return got


def main():
    out = {"tree": TREE, "loose": LOOSE}
    with tempfile.TemporaryDirectory(prefix="rawin_") as tmp:
        root = Path(tmp) / "input"
        for d, files in TREE.items():
            (root / d).mkdir(parents=True)
            for f in files:
                (root / d / f).write_bytes(b"")
        for f in LOOSE:
            (root / f).write_bytes(b"")
        t = process_input(root)
        out["folder"] = [[r["sample"], sorted(r["labels"]), [str(Path(f).relative_to(root)) for f in r["files"]]]
                         for _, r in t.iterrows()]
        csv = Path(tmp) / "table" / "samples.csv"
        csv.parent.mkdir()
        out["csv_text"] = ("labels,sample,files\n" "fam1;gen1,sA,sA_R1.fq;sA_R2.fq\n" "fam2,sB,reads/sB.fq.gz\n"
                           "fam1,sA,sA_extra.fq\n")
        csv.write_text(out["csv_text"])
        t = process_input(csv)
        out["csv"] = [[r["sample"], sorted(r["labels"]), [str(Path(f).relative_to(csv.parent)) for f in r["files"]]]
                      for _, r in t.iterrows()]
    out["pairing"] = {name: {"files": files, "reads": pairing(files)} for name, files in PAIRINGS.items()}
    out["budget"] = []
    for name, max_bp, info in BUDGETS:
        fi = {k: [{"file": f, "avg_length": a, "total_reads": n} for f, a, n in v] for k, v in info.items()}
        out["budget"].append({"name": name, "max_bp": max_bp, "files_info": fi,
                              "take": ref_image.calculate_reads_needed(fi, max_bp)})
    dst = ROOT / "tests" / "golden" / "raw_input_cases.json"
    dst.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
