"""`--gpu-png` against the same run without it, on tiny inputs: the same file names and folders, decoded pixels and
text chunks equal, stats.csv with the same columns and the same rows apart from the times, predictions.csv identical.
The files' bytes are not compared: they are not PIL's."""
import gzip
import os
import random
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def run(argv, cwd):
    """`python -m varkoder_amd ...` in this process (a run is one engine; no second interpreter to start)."""
    from varkoder_amd import cli
    old = os.getcwd()
    os.chdir(cwd)
    try:
        cli.main([str(a) for a in argv])
    finally:
        os.chdir(old)


def reads(seed, bases):
    rng = random.Random(seed)
    parts, total, i = [], 0, 0
    while total < bases:
        n = rng.choice((150, 150, 150, 120, 640))
        parts.append(f"@s{seed}.{i} extra\n{''.join(rng.choice('ACGT') for _ in range(n))}\n+\n{'G' * n}\n")
        total += n
        i += 1
    return "".join(parts).encode()


def sequence(seed, n):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def same_images(a, b):
    """the same relative paths under both folders; pixels, mode and text chunks equal; the second folder's files are in
    the GPU's format (one IDAT, filter 0 in every row)"""
    import zlib
    from PIL import Image
    import png_cases as P
    fa = {str(p.relative_to(a)): p for p in Path(a).rglob("*.png")}
    fb = {str(p.relative_to(b)): p for p in Path(b).rglob("*.png")}
    assert fa and sorted(fa) == sorted(fb)
    for name in fa:
        Image.open(fb[name]).verify()
        ia, ib = Image.open(fa[name]), Image.open(fb[name])
        assert ia.mode == ib.mode == "L" and np.array_equal(np.array(ia), np.array(ib)), name
        assert ia.text == ib.text and list(ia.text) == list(ib.text), name
        P.same_file_but_idat(fb[name].read_bytes(), fa[name].read_bytes())
        raw = zlib.decompress(dict(P.file_chunks(fb[name].read_bytes()))[b"IDAT"])
        assert raw == P.raw_stream(np.array(ib)), name
    return sorted(fa)


def same_stats(a, b):
    import pandas as pd
    sa, sb = pd.read_csv(a), pd.read_csv(b)
    assert list(sa.columns) == list(sb.columns) and len(sa) == len(sb)
    keep = [c for c in sa.columns if not c.endswith("_time")]
    assert keep and len(keep) < len(sa.columns)
    pd.testing.assert_frame_equal(sa[keep], sb[keep], check_exact=True)


@pytest.mark.parametrize("k,mapping", [(7, "cgr"), (7, "varKode"), (9, "cgr")])
def test_default_entry(tmp_path, k, mapping):
    d = tmp_path / "int" / "split_fastqs"
    d.mkdir(parents=True)
    for i, (s, kb) in enumerate((("sA", 10), ("sA", 20), ("sB", 10))):
        (d / f"{s}@{str(kb).rjust(8, '0')}K.fq.gz").write_bytes(gzip.compress(reads(40 + i, kb * 1000), 1))
    (tmp_path / "labels.csv").write_text("sample,labels\nsA,genus:Aus;species:Aus bus\nsB,λ-clade\n")
    common = ["image", "int", "-k", k, "-p", mapping, "--labels-csv", "labels.csv"]
    run(common + ["-o", "A", "-f", "A.csv"], tmp_path)
    run(common + ["-o", "B", "-f", "B.csv", "--gpu-png"], tmp_path)
    assert len(same_images(tmp_path / "A", tmp_path / "B")) == 3
    same_stats(tmp_path / "A.csv", tmp_path / "B.csv")


def test_from_raw_with_a_two_step_ladder(tmp_path):
    for i, s in enumerate(("rawA", "rawB")):
        d = tmp_path / "raw" / "taxon" / s
        d.mkdir(parents=True)
        (d / f"{s}.fq").write_bytes(reads(60 + i, 30000))
    common = ["image", "--from-raw", "raw", "-R", "7", "-m", "5K", "-M", "10K", "-k", "7"]
    run(common + ["-o", "A", "-f", "A.csv"], tmp_path)
    run(common + ["-o", "B", "-f", "B.csv", "--gpu-png"], tmp_path)
    assert len(same_images(tmp_path / "A", tmp_path / "B")) == 4
    same_stats(tmp_path / "A.csv", tmp_path / "B.csv")


def test_from_fasta_windows(tmp_path):
    (tmp_path / "fa").mkdir()
    (tmp_path / "fa" / "asm.fa").write_text(f">one\n{sequence(1, 25000)}\n>two\n{sequence(2, 12000)}\n")
    common = ["image", "fa", "--from-fasta", "--windows", "--window-length", "10000", "--window-step", "5000", "-k", "7"]
    run(common + ["-o", "A", "-f", "A.csv"], tmp_path)
    run(common + ["-o", "B", "-f", "B.csv", "--gpu-png"], tmp_path)
    assert len(same_images(tmp_path / "A", tmp_path / "B")) == 5
    same_stats(tmp_path / "A.csv", tmp_path / "B.csv")


def test_query_from_fasta_keeps_the_same_images_and_predicts_the_same(tmp_path):
    import torch

    class Tiny(torch.nn.Module):   # (the seeded model of tests/test_query.py)
        def __init__(self):
            super().__init__()
            self.pool = torch.nn.AdaptiveAvgPool2d(6)
            self.fc = torch.nn.Linear(3 * 36, 4)

        def forward(self, x):
            return self.fc(self.pool(x).flatten(1))
    torch.manual_seed(3)
    m = Tiny()
    with torch.no_grad():
        m.fc.weight.mul_(40.0)
    torch.jit.script(m).save(str(tmp_path / "m.pt"))
    (tmp_path / "vocab.txt").write_text("a\nb\nc\nd\n")
    (tmp_path / "fa").mkdir()
    for i, s in enumerate(("x", "y", "z")):
        (tmp_path / "fa" / f"{s}.fa").write_text(f">r\n{sequence(10 + i, 9000 + 1000 * i)}\n")
    common = ["query", "-l", "m.pt", "--vocab", "vocab.txt", "-k", "7", "-p", "cgr", "fa"]
    run(common + ["A", "--from-fasta", "-m", "-P", "-b", "2"], tmp_path)
    run(common + ["B", "--from-fasta", "-m", "-P", "-b", "2", "--gpu-png"], tmp_path)
    assert len(same_images(tmp_path / "A" / "query_images", tmp_path / "B" / "query_images")) == 3
    a = (tmp_path / "A" / "predictions.csv").read_text().replace("A/query_images/", "OUT/query_images/")   # (the folder's own name)
    b = (tmp_path / "B" / "predictions.csv").read_text().replace("B/query_images/", "OUT/query_images/")
    assert a == b and a.count("\n") == 4 and a.count("OUT/query_images/") == 3
