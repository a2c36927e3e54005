"""`query --from-raw` on the MI355X: the read-length heads kernel (vk_clean_heads_device through
ImageEngine.clean_heads) against rawinput.avg_read_length's sums, and the command end to end against tests/clean_ref.py,
against today's `query` on the cleaned reads it leaves, and against `query -I` on the images it keeps."""
import gzip
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_ref as R  # noqa: E402

from varkoder_amd import rawinput  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CHUNK = 16384   # kClChunk: the bytes a workgroup of the heads kernel takes per round


@pytest.fixture(scope="module")
def eng():
    from varkoder_amd.engine import ImageEngine
    e = ImageEngine(k=7, mapping="cgr", device=0)
    yield e
    e.close()


# ---- the heads kernel ---------------------------------------------------------------------------

def head_sums(text, sample_size=10000):
    """avg_read_length's `total` and `n` (the same loop; it returns only their quotient)."""
    total = n = 0
    for i, line in enumerate(text.split(b"\n")):
        if i % 4 == 1:
            total += len(line.strip())
            n += 1
            if n >= sample_size:
                break
    assert (total / n if n else 0) == rawinput.avg_read_length(text, sample_size)
    return total, n


def check_heads(eng, texts, sample_sizes=(10000,)):
    dev, offs, lens = eng.upload(texts)
    for ss in sample_sizes:
        totals, counted = eng.clean_heads(dev, offs, lens, ss)
        want = [head_sums(t, ss) for t in texts]
        got = list(zip(totals.tolist(), counted.tolist()))
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (ss, bad[:5])


def records_text(rng, n, lo=30, hi=250, eol=b"\n"):
    lens = rng.integers(lo, hi + 1, n)
    seq = b"ACGT" * (hi // 4 + 1)
    return b"".join(b"@r%d" % i + eol + seq[:L] + eol + b"+" + eol + b"I" * L + eol for i, L in enumerate(lens.tolist()))


def test_heads_around_the_sample_size(eng):
    rng = np.random.default_rng(1)
    check_heads(eng, [records_text(rng, n) for n in (9999, 10000, 10001, 1, 0, 25000)], (10000, 1, 2, 9999))


def test_heads_line_shapes(eng):
    rng = np.random.default_rng(2)
    body = records_text(rng, 50)
    texts = [
        records_text(rng, 300, eol=b"\r\n"),                                   # CRLF lines
        b"@a\nACGT  \t\n+\nIIII\n@b\n \tACGTA\t \n+\nIIIII\n@c\nAC GT\x0b\x0c\n+\nIIIII\n",   # blanks at the ends, one inside
        b"@a\n\n+\n\n@b\nACG\n+\nIII\n",                                       # an empty sequence line
        b"@a\n \t \n+\nI\n@b\n\r\n+\n\n@c\nAC\n+\nII\n",                       # sequence lines of whitespace only
        b"@a\nACGT\n+\nIIII\n@b\nACGTACGT",                                    # no final newline, ends in a sequence line
        b"@a\nACGT\n+\nIIII\n@b\nACGTAC \t",                                   # ... with blanks at its end
        b"@a\nACGT\n+\nIIII\n@b\n",                                            # ends where a sequence line would begin
        b"@a\nACGT\n+\nIIII\n@b\n  ",                                          # ... with blanks only
        b"@a\nACGT\n+\nIIII",                                                  # ends in a quality line
        b"@a",                                                                 # no newline at all
        b"@a\n",
        b"\n\n\n\n\n\n",
        b"ACGT",
        b"",                                                                   # an empty file
        body + b"@last\nACGTACGTAC",
        body,
    ]
    check_heads(eng, texts, (10000, 1, 3, 51, 52))


def straddling(rng, nbefore, seq_len=150):
    """nbefore records, then one whose sequence line starts 50 bytes ahead of a chunk boundary, then a few more."""
    head = records_text(rng, nbefore)
    boundary = (len(head) + 64 + CHUNK - 1) // CHUNK * CHUNK
    name = b"@" + b"x" * (boundary - 50 - len(head) - 2)
    text = head + name + b"\n" + b"ACGT" * 40 + b"\n+\n" + b"I" * 160 + b"\n" + records_text(rng, 5)
    start = len(head) + len(name) + 1
    assert start < boundary < start + 160 and boundary % CHUNK == 0
    return text


def test_heads_last_sampled_line_straddles_a_chunk(eng):
    rng = np.random.default_rng(3)
    texts = [straddling(rng, 9999), straddling(rng, 0), straddling(rng, 9998)]
    # and the newline that ends the 10,000th sequence line as the last / first byte of a chunk
    for shift in (0, 1):
        head = records_text(rng, 9999)
        boundary = (len(head) + 300 + CHUNK - 1) // CHUNK * CHUNK
        name = b"@" + b"y" * (boundary - shift - 102 - len(head))
        t = head + name + b"\n" + b"A" * 100 + b"\n+\n" + b"I" * 100 + b"\n" + records_text(rng, 3)
        assert t[boundary - shift] == 10 and t[boundary - shift - 1] == 65
        texts.append(t)
    check_heads(eng, texts, (10000, 1))


def test_heads_one_large_file_beside_many_tiny_ones(eng):
    rng = np.random.default_rng(4)
    block = records_text(rng, 20000)
    big = block * ((64 << 20) // len(block) + 1)
    assert len(big) >= 64 << 20
    tiny = [records_text(rng, int(n)) for n in rng.integers(0, 6, 300)]
    check_heads(eng, tiny[:150] + [big] + tiny[150:], (10000,))


def test_heads_fuzz(eng):
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"ACGTN \t\r\n\n\n\x0b\x0c@+I", dtype=np.uint8)
    texts = [bytes(alphabet[rng.integers(0, len(alphabet), int(n))]) for n in rng.integers(0, 400, 200)]
    check_heads(eng, texts, (10000, 1, 2, 7))


def test_heads_refuses_a_sample_size_of_zero(eng):
    from varkoder_amd._capi import VkError
    dev, offs, lens = eng.upload([b"@a\nACGT\n+\nIIII\n"])
    with pytest.raises(VkError):
        eng.clean_heads(dev, offs, lens, 0)


# ---- the command --------------------------------------------------------------------------------

def _tiny_model(path, classes):
    """The seeded model tests/test_query.py builds for the `query` command."""
    import torch

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pool = torch.nn.AdaptiveAvgPool2d(6)
            self.fc = torch.nn.Linear(3 * 36, classes)

        def forward(self, x):
            return self.fc(self.pool(x).flatten(1))
    torch.manual_seed(3)
    m = Tiny()
    with torch.no_grad():
        m.fc.weight.mul_(40.0)
    torch.jit.script(m).save(str(path))
    return m


VOCAB = ["a", "b", "c", "d"]

# Sample names are chosen so that their order by name (the input table's: seeds go by its row index) is the order of
# the files `<sample>.fq.gz` by name (today's `query` on clean_reads seeds by that one): qa < qb < qc < qd either way.
# synth_set: fragments shorter than the reads (adapter read-through, then a poly-G tail), N bases, exact duplicates.
SETS = {"qa": R.synth_set(61, 3000, 0), "qb": R.synth_set(62, 0, 4000), "qc": R.synth_set(63, 1500, 1000),
        "qd": R.synth_set(64, 0, 2500, L=101)}


def write_raw(root, layout):
    """{sample: {"R1" | "R2" | "unpaired": (path, records)}}.  folders: a folder per sample (pairs as .fq.gz, single
    reads as plain text, qc with both); flat: a file per sample, so only the single-end sets."""
    root.mkdir()
    plan = {}
    for s, (r1, r2, se) in SETS.items():
        if layout == "flat":
            if r1:
                continue
            p = root / (f"{s}.fq.gz" if s == "qb" else f"{s}.v1.fastq")
            p.write_bytes(gzip.compress(R.fq(se)) if p.suffix == ".gz" else R.fq(se))
            plan[s] = {"unpaired": (p, se)}
            continue
        d = root / s
        d.mkdir()
        plan[s] = {}
        if r1:
            for key, recs, tag in (("R1", r1, "1"), ("R2", r2, "2")):
                p = d / f"lib_{tag}.fq.gz"
                p.write_bytes(gzip.compress(R.fq(recs)))
                plan[s][key] = (p, recs)
        if se:
            p = d / "single.fastq"
            p.write_bytes(R.fq(se))
            plan[s]["unpaired"] = (p, se)
    if layout == "folders":
        (root / "loose.fq").write_bytes(R.fq(SETS["qb"][2][:10]))   # beside sample folders: ignored
    return plan


def expected_clean(files, max_bp, F, T, adapter, merge, dedup):
    """clean_ref's text for one sample's files under the read budget of calculate_reads_needed."""
    info = {"unpaired": [], "R1": [], "R2": []}
    for key, (p, recs) in files.items():
        text = R.fq(recs)
        avg = round(rawinput.avg_read_length(text)) if max_bp is not None else 0
        info[key].append({"file": str(p), "avg_length": avg, "total_reads": len(recs)})
    take = rawinput.reads_needed(info, max_bp)
    part = {key: recs[:take.get(str(p), 0)] for key, (p, recs) in files.items()}
    return R.clean_sample(part.get("R1", []), part.get("R2", []), part.get("unpaired", []), F=F, T=T, adapter=adapter,
                          merge=merge, dedup=dedup)[0]


def query(tmp_path, *args):
    from varkoder_amd import cli
    cli.main(["query", "-l", str(tmp_path / "m.pt"), "--vocab", str(tmp_path / "vocab.txt"), "-k", "7", "-p", "cgr"] +
             [str(a) for a in args])


def model_files(tmp_path):
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    _tiny_model(tmp_path / "m.pt", len(VOCAB))


@pytest.mark.parametrize("layout,max_bp,flags", [("folders", "200M", []), ("flat", "200M", []),
                                                 ("folders", "40K", []), ("folders", "200M", ["-a", "-r", "-D", "-T", "0,0"])])
def test_query_from_raw_end_to_end(tmp_path, layout, max_bp, flags):
    import pandas as pd   # (float_precision="round_trip": the default parser may be an ulp off what the file says)
    from PIL import Image
    from varkoder_amd.cli import parse_size
    from varkoder_amd.rawinput import curves_sd
    model_files(tmp_path)
    plan = write_raw(tmp_path / "raw", layout)
    samples = sorted(plan)
    common = ["-R", "5", "-M", max_bp, "-b", "2", "-P"]
    query(tmp_path, tmp_path / "raw", tmp_path / "out_raw", "--from-raw", "-i", tmp_path / "int", "--keep-images", *common, *flags)
    # 1. the cleaned reads are clean_ref's for each sample's files and budget
    F, T = (0, 0) if flags else (10, 10)
    on = not flags
    clean = tmp_path / "int" / "clean_reads"
    for s in samples:
        want = expected_clean(plan[s], parse_size(max_bp), F, T, on, on, on)
        assert gzip.decompress((clean / f"{s}.fq.gz").read_bytes()) == want, s
    assert sorted(p.name for p in clean.glob("*.fq.gz")) == [f"{s}.fq.gz" for s in samples]
    assert not (tmp_path / "out_raw" / "stats.csv").exists() and not Path("stats.csv").exists()
    a = pd.read_csv(tmp_path / "out_raw" / "predictions.csv", float_precision="round_trip")
    assert list(a["sample_id"]) == samples and set(a["actual_labels"]) == {"query"}
    if max_bp == "40K":   # the rung is a subsample: every sample holds more than that after cleaning
        assert list(a["query_basepairs"]) == [40000] * len(samples)
    # 2. today's query on that clean_reads folder: the same pixels, the same predictions
    query(tmp_path, tmp_path / "int", tmp_path / "out_clean", "-m", *common)
    b = pd.read_csv(tmp_path / "out_clean" / "predictions.csv", float_precision="round_trip")
    drop = ["varKode_image_path", "actual_labels", "basefrequency_sd"]
    pd.testing.assert_frame_equal(a.drop(columns=drop), b.drop(columns=drop), check_exact=True)
    names = sorted(p.name for p in (tmp_path / "out_raw" / "query_images").glob("*.png"))
    assert len(names) == len(samples) and names == sorted(p.name for p in (tmp_path / "out_clean" / "query_images").glob("*.png"))
    assert list(a["varKode_image_path"]) == [str(tmp_path / "out_raw" / "query_images" / n) for n in names]
    for n in names:
        x, y = Image.open(tmp_path / "out_raw" / "query_images" / n), Image.open(tmp_path / "out_clean" / "query_images" / n)
        assert np.array_equal(np.array(x), np.array(y)), n
        assert x.info["varkoderKeywords"] == "query"
    # 3. a query of the kept images: every column but the path
    query(tmp_path, tmp_path / "out_raw" / "query_images", tmp_path / "out_img", "-I", "-b", "2", "-P")
    c = pd.read_csv(tmp_path / "out_img" / "predictions.csv", float_precision="round_trip")
    assert list(c["varKode_image_path"]) == list(a["varKode_image_path"])
    pd.testing.assert_frame_equal(a.drop(columns=["varKode_image_path"]), c.drop(columns=["varKode_image_path"]), check_exact=True)
    # 4. the figure is that of the report written beside the cleaned reads
    for s, sd in zip(a["sample_id"], a["basefrequency_sd"]):
        curves = json.loads((clean / f"{s}_fastp_gpu.json").read_text())["read1_after_filtering"]["content_curves"]
        assert sd == curves_sd(curves) and sd > 0, s
    # 5. a second run takes the cleaned reads as they are and predicts the same
    query(tmp_path, tmp_path / "raw", tmp_path / "out_again", "--from-raw", "-i", tmp_path / "int", *common, *flags)
    d = pd.read_csv(tmp_path / "out_again" / "predictions.csv", float_precision="round_trip")
    pd.testing.assert_frame_equal(a.drop(columns=["varKode_image_path"]), d.drop(columns=["varKode_image_path"]), check_exact=True)


def test_a_corrupt_sample_is_reported_and_skipped(tmp_path, capsys):
    import pandas as pd
    model_files(tmp_path)
    raw = tmp_path / "raw"
    raw.mkdir()
    se = SETS["qb"][2]
    (raw / "good1.fq").write_bytes(R.fq(se[:1500]))
    (raw / "bad.fq").write_bytes(R.fq(se[:3]) + b"@q\nACGT\n+\nIII\n" + R.fq(se[3:50]))   # quality shorter than the sequence
    (raw / "good2.fq.gz").write_bytes(gzip.compress(R.fq(se[1500:3500])))
    query(tmp_path, raw, tmp_path / "out", "--from-raw", "-P")   # (returns: the command's exit code is 0)
    err = capsys.readouterr().err
    assert "CLEAN FAIL:" in err and "bad.fq" in err
    df = pd.read_csv(tmp_path / "out" / "predictions.csv", float_precision="round_trip")
    assert list(df["sample_id"]) == ["good1", "good2"] and np.isfinite(df[VOCAB].to_numpy()).all()


def test_query_from_raw_at_world_two_equals_single_rank(tmp_path):
    """Both ranks on cuda:0, samples dealt by size.  -b 1: every forward has one row on either run, so the rows do
    not depend on which samples share a rank and the files can be compared as they are."""
    import pandas as pd
    model_files(tmp_path)
    write_raw(tmp_path / "raw", "folders")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    common = ["query", "-l", str(tmp_path / "m.pt"), "--vocab", str(tmp_path / "vocab.txt"), "-k", "7", "-p", "cgr", "-P",
              "-R", "9", "-M", "100K", "-b", "1", "--from-raw", str(tmp_path / "raw")]
    one = subprocess.run([sys.executable, "-m", "varkoder_amd"] + common + [str(tmp_path / "out1")],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert one.returncode == 0, one.stderr[-2000:]
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "varkoder_amd"] + common +
                         [str(tmp_path / "out2")], capture_output=True, text=True, timeout=420, cwd=ROOT,
                         env=dict(env, VARKODER_AMD_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert two.returncode == 0, two.stderr[-3000:]
    a, b = (pd.read_csv(tmp_path / d / "predictions.csv", float_precision="round_trip") for d in ("out1", "out2"))
    assert list(a["sample_id"]) == sorted(SETS)
    pd.testing.assert_frame_equal(a, b, check_exact=True)
    text = [(tmp_path / d / "predictions.csv").read_text().replace(str(tmp_path / d), "") for d in ("out1", "out2")]
    assert text[0] == text[1]
