"""`--from-fasta` on the GPU: vk_count_fasta_device against tests/fasta_ref.py (histograms, sequence bytes and
statuses equal, k = 5..9), with VKIMG_FASTA_UNIT_BYTES small in one engine and at its default in another; then .fa.gz,
the commands and the dsk shim.  Every case of fasta_cases.py runs at every k."""
import functools
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
KS = FC.KS
UNITS = ("small", "default")


@pytest.fixture(scope="module")
def fa_engines():
    """(k, "small" | "default") -> an ImageEngine whose context was made with VKIMG_FASTA_UNIT_BYTES = 256 or unset."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(k, unit):
        if (k, unit) not in cache:
            old = os.environ.pop("VKIMG_FASTA_UNIT_BYTES", None)
            try:
                if unit == "small":
                    os.environ["VKIMG_FASTA_UNIT_BYTES"] = str(FC.SMALL_UNIT)
                cache[(k, unit)] = ImageEngine(k=k, mapping="cgr", device=0)
            finally:
                os.environ.pop("VKIMG_FASTA_UNIT_BYTES", None)
                if old is not None:
                    os.environ["VKIMG_FASTA_UNIT_BYTES"] = old
        return cache[(k, unit)]
    yield get
    for e in cache.values():
        e.close()


@functools.lru_cache(maxsize=None)
def expected(group, k):
    """(cases, [(hist, status, bases)]) of a group of fasta_cases.py: computed once, shared, left unchanged."""
    cases = {"lines": FC.line_cases, "headers": FC.header_cases, "breaks": FC.break_cases, "poly_a": lambda k: FC.poly_a(),
             "seams_small": lambda k: FC.seam_cases(k, FC.SMALL_UNIT), "seams_unit": lambda k: FC.seam_cases(k, FC.UNIT),
             "seams_span": FC.span_seam_cases, "batch": FC.batch_cases}[group](k)
    return cases, [FR.count(data, k) for _, data in cases]


def gpu_count(eng, samples):
    dev, offs, lens = eng.upload(samples)
    hist, status, bases = eng.count_fasta(dev, offs, lens)
    return hist.cpu().numpy().view(np.uint32), status.cpu().numpy().view(np.uint32), bases.cpu().numpy()


def check_group(eng, group, k):
    cases, want = expected(group, k)
    hist, status, bases = gpu_count(eng, [d for _, d in cases])
    for i, ((name, _), (wh, ws, wb)) in enumerate(zip(cases, want)):
        assert int(status[i]) == ws, name
        assert int(bases[i]) == wb, name
        if ws == 0:
            assert np.array_equal(hist[i], wh), name


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("group", ("lines", "headers", "breaks", "poly_a", "batch"))
def test_count_equals_the_rule(fa_engines, group, k, unit):
    """Line widths 1, 2, 3, k - 1, k, 60, 61, unwrapped, CRLF, no final newline, empty lines, stray \\r; headers (ACGT
    text, '>', 70,000 bytes, no sequence, two in a row, '>' inside a sequence line); breaks (N runs of 1 and k, lower
    case, IUPAC, runs of k - 1 and k bases, poly-A of 1 MB); the batch of 64 at every 16-byte residue with an empty
    sample and a FASTQ (VK_ST_BAD_START) among exact neighbours."""
    check_group(fa_engines(k, unit), group, k)


@pytest.mark.parametrize("k", KS)
def test_seams_small_unit(fa_engines, k):
    """Header length 0..unit + 64 in steps of one, unit = 256: record start, line ends, a run of line ends, a second
    header and every window start fall on lane, wave-of-lanes and workgroup seams."""
    check_group(fa_engines(k, "small"), "seams_small", k)
    check_group(fa_engines(k, "default"), "seams_small", k)


@pytest.mark.parametrize("k", KS)
def test_seams_default_unit(fa_engines, k):
    """The same at the default: steps of one near a unit's ends, coarser between; and around the seam between two
    workgroups."""
    check_group(fa_engines(k, "default"), "seams_unit", k)
    check_group(fa_engines(k, "default"), "seams_span", k)
    check_group(fa_engines(k, "small"), "seams_span", k)


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
def test_wrapped_equals_unwrapped(fa_engines, k, unit):
    s = FC.seq(77, 50000, b"ACGTACGTACGTN")
    recs = [(b"a", s[:30011]), (b"b", s[30011:])]
    hist, status, bases = gpu_count(fa_engines(k, unit), [FC.fasta(recs, None), FC.fasta(recs, 60), FC.fasta(recs, 70, b"\r\n")])
    assert status.tolist() == [0, 0, 0] and bases.tolist() == [50000] * 3
    assert np.array_equal(hist[0], hist[1]) and np.array_equal(hist[0], hist[2])
    assert np.array_equal(hist[0], FR.count(FC.fasta(recs, 60), k)[0])


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
def test_host_call_and_gz(fa_engines, tmp_path, k, unit):
    """count_fasta_host on one sample; a .fa.gz through upload_files gives the plain file's histogram."""
    eng = fa_engines(k, unit)
    data = FC.fasta([(b"chr1 x", FC.seq(5, 40000)), (b"chr2", FC.seq(6, 25000, b"ACGTN"))], 60)
    want = FR.count(data, k)
    h, st, nb = eng.count_fasta_host(data)
    assert st == 0 and nb == want[2] and np.array_equal(h, want[0])
    h0, st0, nb0 = eng.count_fasta_host(b"")
    assert st0 == 0 and nb0 == 0 and not h0.any()
    plain, gz = tmp_path / "a.fa", tmp_path / "b.fa.gz"
    plain.write_bytes(data)
    with gzip.open(gz, "wb") as f:
        f.write(data)
    dev, offs, lens = eng.upload_files([str(plain), str(gz)])
    assert lens.tolist() == [len(data)] * 2
    hist, status, bases = eng.count_fasta(dev, offs, lens)
    hist = hist.cpu().numpy().view(np.uint32)
    assert status.cpu().tolist() == [0, 0] and bases.cpu().tolist() == [want[2]] * 2
    assert np.array_equal(hist[0], want[0]) and np.array_equal(hist[1], want[0])


@pytest.mark.parametrize("k", KS)
def test_nothing_moved_fastq_count_still_refuses_fasta(fa_engines, k):
    """The existing pin (test_gpu_parity.py::test_bad_framing_sets_status), for the new engine objects."""
    data = FC.fasta([(b"r", FC.seq(3, 500))], 60)
    for unit in UNITS:
        _, st = fa_engines(k, unit).count_host(data)
        assert st & 1


# ---- whole commands -------------------------------------------------------------------------------

def command_files(root):
    """Three small FASTA files (one .gz, one CRLF and unwrapped, one with an empty record and lower case), a file with
    a bad start and one without a base; {sample: bytes} of the good ones."""
    src = root / "fasta"
    src.mkdir()
    good = {
        "mito": FC.fasta([(b"NC_000001 mitochondrion", FC.seq(901, 16569))], 70),
        "plastid.v2": FC.fasta([(b"contig1", FC.seq(902, 40000, b"ACGTacgtN")), (b"empty", b""), (b"contig2", FC.seq(903, 9000))], None, b"\r\n"),
        "scaffolds": FC.fasta([(b"s%d" % i, FC.seq(910 + i, 700 + 37 * i)) for i in range(40)], 60),
    }
    (src / "mito.fa").write_bytes(good["mito"])
    (src / "plastid.v2.fasta").write_bytes(good["plastid.v2"])
    (src / "scaffolds.fna.gz").write_bytes(gzip.compress(good["scaffolds"]))
    (src / "reads.fa").write_bytes(b"@r\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")
    (src / "nobase.fa").write_bytes(b">only a header\n")
    (src / "notes.txt").write_bytes(b"not a sample\n")
    return src, good


@pytest.mark.parametrize("k,mapping", [(7, "cgr"), (9, "varKode"), (5, "cgr")])
def test_image_from_fasta_command(tmp_path, k, mapping):
    import pandas as pd
    from PIL import Image
    from oracle import oracle
    from varkoder_amd import cli
    from varkoder_amd.mapping import pixel_lut, side
    src, good = command_files(tmp_path)
    (tmp_path / "labels.csv").write_text("sample,labels\nmito,genus:Homo;family:Hominidae\nscaffolds,genus:Zea\n")
    out = tmp_path / "images"
    cli.main(["image", str(src), "--from-fasta", "-k", str(k), "-p", mapping, "-o", str(out), "-f", str(tmp_path / "stats.csv"),
              "-t", "--labels-csv", str(tmp_path / "labels.csv")])
    npix = side(k, mapping) ** 2
    pix = oracle.cgr_lut(k) if mapping == "cgr" else np.ascontiguousarray(pixel_lut(k, mapping), dtype=np.uint32)
    names = {}
    for s, data in good.items():
        nb = FR.bases(data)
        names[s] = f"{s}@{str(nb // 1000).rjust(8, '0')}K+{mapping}+k{k}.png"
        want, _, st = oracle.fastq_to_image(FR.to_fastq(data), k, pix, npix)
        assert st == 0
        im = Image.open(out / names[s])
        assert np.array_equal(np.array(im).ravel(), want), s
        assert im.info["varkoderBaseFreqSd"] == "0" and im.info["varkoderLowQualityFlag"] == "False"
    assert sorted(p.name for p in out.glob("*.png")) == sorted(names.values())
    assert Image.open(out / names["mito"]).info["varkoderKeywords"] == "genus:Homo;family:Hominidae"
    stats = pd.read_csv(tmp_path / "stats.csv").set_index("sample")
    assert sorted(stats.index) == ["mito", "nobase", "plastid.v2", "reads", "scaffolds"]
    assert {f"{k}mer_counting_time", f"k{k}_img_time", "base_frequencies_sd", "failed_step"} == set(stats.columns)
    for s in good:
        assert stats.loc[s, f"{k}mer_counting_time"] > 0 and stats.loc[s, f"k{k}_img_time"] > 0
        assert stats.loc[s, "base_frequencies_sd"] == 0 and pd.isna(stats.loc[s, "failed_step"])
    assert stats.loc["reads", "failed_step"] == "image" and stats.loc["nobase", "failed_step"] == "image"
    lt = pd.read_csv(out / "labels.csv", dtype=str).fillna("")
    assert list(lt["sample"]) == ["mito", "nobase", "plastid.v2", "reads", "scaffolds"]
    assert list(lt["labels"]) == ["genus:Homo;family:Hominidae", "", "", "", "genus:Zea"]
    assert set(lt["possible_low_quality"]) == {"False"}


def test_query_from_fasta_command(tmp_path):
    import pandas as pd
    import torch
    from varkoder_amd import cli

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

    def query(_, *args):
        cli.main(["query", "-l", str(tmp_path / "m.pt"), "--vocab", str(tmp_path / "vocab.txt"), "-k", "7", "-p", "cgr"] +
                 [str(a) for a in args])
    src, good = command_files(tmp_path)
    query(tmp_path, src, tmp_path / "out", "--from-fasta", "-m", "-P", "-b", "2")
    a = pd.read_csv(tmp_path / "out" / "predictions.csv", float_precision="round_trip")
    assert list(a["sample_id"]) == sorted(good)
    assert list(a["query_basepairs"]) == [FR.bases(good[s]) // 1000 * 1000 for s in sorted(good)]
    kept = sorted(p.name for p in (tmp_path / "out" / "query_images").glob("*.png"))
    assert kept == sorted(f"{s}@{str(FR.bases(d) // 1000).rjust(8, '0')}K+cgr+k7.png" for s, d in good.items())
    query(tmp_path, tmp_path / "out" / "query_images", tmp_path / "out_img", "-I", "-P", "-b", "2")
    b = pd.read_csv(tmp_path / "out_img" / "predictions.csv", float_precision="round_trip")
    assert list(b["varKode_image_path"]) == list(a["varKode_image_path"])
    pd.testing.assert_frame_equal(a.drop(columns=["varKode_image_path"]), b.drop(columns=["varKode_image_path"]), check_exact=True)


@pytest.mark.parametrize("k,gz", [(7, False), (9, True)])
def test_dsk_shim_on_a_fasta_file(tmp_path, k, gz):
    from varkoder_amd import formats, shims
    data = FC.fasta([(b"chrM", FC.seq(950, 16000, b"ACGTN")), (b"chrC", FC.seq(951, 5000))], 60)
    path = tmp_path / ("in.fa.gz" if gz else "in.fa")
    path.write_bytes(gzip.compress(data) if gz else data)
    r = subprocess.run([os.path.join(shims.BIN_DIR, "dsk"), "-nb-cores", "1", "-kmer-size", str(k), "-abundance-min", "1", "-file",
                        str(path), "-out-tmp", str(tmp_path), "-out", str(tmp_path / f"in+k{k}.fq.h5")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(shims.BIN_DIR, "dsk2ascii"), "-c", "-file", str(tmp_path / f"in+k{k}.fq.h5"), "-nb-cores", "1",
                        "-out", str(tmp_path / "dsk.txt"), "-verbose", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == formats.dsk_text(FR.count(data, k)[0], k, "gatb")
