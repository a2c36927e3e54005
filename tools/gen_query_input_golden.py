#!/usr/bin/env python3
"""Golden cases for `query --from-raw`'s input table, made by running the reference's own process_input with
is_query=True (core/utils.py:340-383, 401-409) unmodified on small trees of empty files.  Build-container only (needs
the reference tree, imported through oracle/ref_harness.py).  Writes tests/golden/query_input_cases.json -- recorded
results only; varkoder_amd/rawinput.py must reproduce every case (tests/test_query_input.py).

A case: `dirs` (folders to make), `files` (empty files), `links` ({link: target folder}, both relative to the input
folder) and either `table` = [[sample, labels, files relative to the input folder]] or `exception` = the type and
text of what the reference raised.

Usage:  python tools/gen_query_input_golden.py
"""
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import ref_harness  # noqa: E402

ref_harness.install()
from varKoder.core.utils import process_input  # noqa: E402

CASES = [
    # no sub-folders: every FASTQ file is a sample, named up to the first '.'; other files are left out
    {"name": "flat", "files": ["s1.fq", "s2.fastq.gz", "s3.v2.fq.gz", "notes.txt", "s4.fq.md5"]},
    # paired-looking names are two samples; names that agree up to the first '.' are one
    {"name": "flat_pairs", "files": ["a_1.fq", "a_2.fq", "b.1.fq.gz", "b.2.fq.gz", "c_R1_001.fastq", "c_R2_001.fastq"]},
    # a folder per sample: pairs, singles, a non-FASTQ file
    {"name": "folders", "files": ["sA/sA_R1.fq.gz", "sA/sA_R2.fq.gz", "sB/reads.fastq", "sB/readme.txt",
                                  "sC/x_1.fq", "sC/x_2.fq", "sC/x_single.fq"]},
    # a link to a folder is a sample under the link's name
    {"name": "linked_folder", "files": ["real/r_1.fq", "real/r_2.fq", "elsewhere/e.fq"], "links": {"linked": "elsewhere"}},
    # loose files beside sample folders are ignored, and so is a folder below a sample folder
    {"name": "mixed", "files": ["loose.fq", "loose_2.fastq.gz", "sA/a.fq", "sA/deeper/d.fq", "sB/b.fq.gz"]},
    {"name": "empty", "files": []},
    {"name": "folders_without_reads", "files": ["sA/readme.txt"], "dirs": ["sB"]},
]


def run(case):
    with tempfile.TemporaryDirectory(prefix="queryin_") as tmp:
        root = Path(tmp) / "input"
        root.mkdir()
        for d in case.get("dirs", []):
            (root / d).mkdir(parents=True)
        for f in case["files"]:
            (root / f).parent.mkdir(parents=True, exist_ok=True)
            (root / f).write_bytes(b"")
        for link, target in case.get("links", {}).items():
            (root / link).symlink_to(root / target, target_is_directory=True)
        try:
            t = process_input(root, is_query=True)
        except Exception as e:   # noqa: BLE001 -- the case records it
            return {"exception": {"type": type(e).__name__, "text": str(e)}}
        return {"table": [[r["sample"], sorted(r["labels"]), [str(Path(f).relative_to(root)) for f in r["files"]]]
                          for _, r in t.iterrows()]}


def main():
    out = {"cases": [dict(case, **run(case)) for case in CASES]}
    dst = ROOT / "tests" / "golden" / "query_input_cases.json"
    dst.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
