"""`image / query --from-fasta --windows` as commands, on the GPU: the pixels of every window equal those of
`--from-fasta --per-record` run on a FASTA whose records are the windows' extended slices (the window's bases and the
k - 1 behind them), for a plain and a gzipped file; names, stats rows, labels.csv and the order of the label lookup;
one predictions.csv row per window in order; and a run without the flag gives what the oracle gives for whole files."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MAPPING, N, S = 7, "cgr", 500, 250
WINDOW_FLAGS = ["--from-fasta", "--windows", "--window-length", N, "--window-step", S]


def nwin(bases):
    return (bases - N) // S + 1 if bases >= N else 0


def command_files(root):
    """A chromosome file (a long record, a short one, one with the first one's id, one all N) and a gzipped assembly
    (CRLF, 60 columns); beside it the folder whose files hold every window's extended slice as a record named
    `<id>__<start>-<end>`.  Returns (folder, folder of slices, [window sample names to be imaged, in order])."""
    src, slices = root / "fasta", root / "slices"
    src.mkdir()
    slices.mkdir()
    chrom = [(b"chr1 Genus species chromosome 1", FC.seq(901, 2600, b"ACGTacgtN")), (b"short", FC.seq(902, 300)),
             (b"chr1 again", FC.seq(903, 1500)), (b"allN", b"N" * 1200)]
    asm = [(b"scaffold_%d cov=%d" % (i, 10 + i), FC.seq(910 + i, 1000 + 333 * i)) for i in range(2)]
    (src / "chr.fa").write_bytes(FC.fasta(chrom, 70))
    (src / "asm.fna.gz").write_bytes(gzip.compress(FC.fasta(asm, 60, b"\r\n")))
    (src / "notes.txt").write_bytes(b"not a sample\n")
    names = []
    for stem, recs, fname in (("asm", [(b"scaffold_0", asm[0][1]), (b"scaffold_1", asm[1][1])], "asm.fa"),
                              ("chr", [(b"chr1", chrom[0][1])], "chr.fa")):
        out = []
        for rid, seq in recs:
            for w in range(nwin(len(seq))):
                wid = b"%s__%d-%d" % (rid, w * S + 1, w * S + N)
                out.append((wid, seq[w * S:min(w * S + N + K - 1, len(seq))]))
                names.append(stem + "__" + wid.decode())
        (slices / fname).write_bytes(FC.fasta(out, 80))
    return src, slices, names


def command(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "varkoder_amd"] + [str(a) for a in args], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def png_of(folder, sample):
    found = list(folder.glob(sample + "@*.png"))
    assert len(found) == 1, (sample, found)
    return found[0]


def test_image_windows_command(tmp_path):
    import pandas as pd
    from PIL import Image
    from oracle import oracle
    src, slices, names = command_files(tmp_path)
    (tmp_path / "labels.csv").write_text("sample,labels\nchr,family:Hominidae\nchr__chr1,genus:Pan\nchr__chr1__251-750,species:Pan_x\n")
    out, ref, plain = tmp_path / "images", tmp_path / "images_slices", tmp_path / "images_plain"
    err = command("image", src, *WINDOW_FLAGS, "-k", K, "-p", MAPPING, "-o", out, "-f", tmp_path / "stats.csv", "-t",
                  "--labels-csv", tmp_path / "labels.csv")
    command("image", slices, "--from-fasta", "--per-record", "--min-record-length", 100, "-k", K, "-p", MAPPING, "-o", ref,
            "-f", tmp_path / "stats_slices.csv")
    assert len(names) == 3 + 4 + 9
    want_png = {s: f"{s}@{str(N // 1000).rjust(8, '0')}K+{MAPPING}+k{K}.png" for s in names}
    assert sorted(p.name for p in out.glob("*.png")) == sorted(want_png.values())
    for s, name in want_png.items():   # the pixels of the window's extended slice given as a record of its own
        assert np.array_equal(np.array(Image.open(out / name)), np.array(Image.open(png_of(ref, s)))), s
    for s in names:
        assert "@" not in s and "+" not in s
    # labels: by window, then by record, then by file
    assert Image.open(out / want_png["chr__chr1__251-750"]).info["varkoderKeywords"] == "species:Pan_x"
    assert Image.open(out / want_png["chr__chr1__1-500"]).info["varkoderKeywords"] == "genus:Pan"
    assert Image.open(out / want_png["asm__scaffold_1__1-500"]).info["varkoderKeywords"] == ""
    stats = pd.read_csv(tmp_path / "stats.csv").set_index("sample")
    all_n = ["chr__allN__%d-%d" % (w * S + 1, w * S + N) for w in range(3)]
    assert sorted(stats.index) == sorted(names + ["chr__chr1#3"] + all_n)
    for s in names:
        assert stats.loc[s, f"{K}mer_counting_time"] > 0 and stats.loc[s, f"k{K}_img_time"] > 0 and pd.isna(stats.loc[s, "failed_step"])
    for s in ["chr__chr1#3"] + all_n:
        assert stats.loc[s, "failed_step"] == "image"
    assert "DUPLICATE RECORD ID, SKIPPING: chr__chr1" in err
    assert f"1 of 4 records shorter than {N} bases passed over, 300 bases behind the last windows of the others" in err
    assert f"0 of 2 records shorter than {N} bases passed over, {(1000 - 1000) + (1333 - 1250)} bases behind" in err
    lt = pd.read_csv(out / "labels.csv", dtype=str).fillna("").set_index("sample")
    assert sorted(lt.index) == sorted(names)
    assert lt.loc["chr__chr1__251-750", "labels"] == "species:Pan_x" and lt.loc["chr__chr1__501-1000", "labels"] == "genus:Pan"
    assert lt.loc["asm__scaffold_0__1-500", "labels"] == ""
    # the step defaults to the length: windows side by side
    command("image", src, "--from-fasta", "--windows", "--window-length", N, "-k", K, "-p", MAPPING, "-o", tmp_path / "side",
            "-f", tmp_path / "stats_side.csv")
    side = sorted(p.name.split("@")[0] for p in (tmp_path / "side").glob("*.png"))
    assert side == sorted(["asm__scaffold_0__1-500", "asm__scaffold_0__501-1000", "asm__scaffold_1__1-500", "asm__scaffold_1__501-1000"] +
                          ["chr__chr1__%d-%d" % (w * N + 1, w * N + N) for w in range(5)])
    for s in ("asm__scaffold_0__501-1000", "chr__chr1__1-500"):   # (windows that both geometries have)
        assert np.array_equal(np.array(Image.open(png_of(tmp_path / "side", s))), np.array(Image.open(out / want_png[s]))), s
    # without the flag: one image per file, the pixels the oracle gives for the file's records
    command("image", src, "--from-fasta", "-k", K, "-p", MAPPING, "-o", plain, "-f", tmp_path / "stats_plain.csv")
    want = {}
    for f, s in ((src / "chr.fa", "chr"), (src / "asm.fna.gz", "asm")):
        data = gzip.decompress(f.read_bytes()) if f.suffix == ".gz" else f.read_bytes()
        img, _, st = oracle.fastq_to_image(FR.to_fastq(data), K, oracle.cgr_lut(K), 4 ** K)
        assert st == 0
        want[f"{s}@{str(FR.bases(data) // 1000).rjust(8, '0')}K+{MAPPING}+k{K}.png"] = img
    assert sorted(p.name for p in plain.glob("*.png")) == sorted(want)
    for name, img in want.items():
        assert np.array_equal(np.array(Image.open(plain / name)).ravel(), img), name
    assert sorted(pd.read_csv(tmp_path / "stats_plain.csv")["sample"]) == ["asm", "chr"]


def test_query_windows_command(tmp_path):
    import pandas as pd
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
    src, slices, names = command_files(tmp_path)
    model = ["-l", tmp_path / "m.pt", "--vocab", tmp_path / "vocab.txt", "-k", K, "-p", MAPPING, "-P", "-b", 2]
    command("query", *model, src, tmp_path / "out", *WINDOW_FLAGS)
    command("query", *model, slices, tmp_path / "out_slices", "--from-fasta", "--per-record", "--min-record-length", 100)
    a = pd.read_csv(tmp_path / "out" / "predictions.csv", float_precision="round_trip")
    b = pd.read_csv(tmp_path / "out_slices" / "predictions.csv", float_precision="round_trip")
    # a row per window: files in order, records in order within each, windows in order within each record
    assert list(a["sample_id"]) == names
    assert list(a["query_basepairs"]) == [N // 1000 * 1000] * len(names)
    pd.testing.assert_frame_equal(a.sort_values("sample_id").reset_index(drop=True), b.sort_values("sample_id").reset_index(drop=True),
                                  check_exact=True)
