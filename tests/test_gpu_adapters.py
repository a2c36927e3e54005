"""Adapters by sequence in step B on the MI355X: vk_clean_detect_device (ImageEngine.detect_adapters) finds what
tests/adapter_ref.detect_adapter finds, per group; vk_clean_adapters_device (ImageEngine.clean(adapters=...)) writes
what adapter_ref.clean_sample_adapters writes, byte for byte, with its stats; without adapters the clean is the one
of before; `image --from-raw --detect-adapters` end to end."""
import gzip
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_ref as A  # noqa: E402
import clean_ref as R  # noqa: E402

from varkoder_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SMALL_RNA = b"TGGAATTCTCGGGTGCCAAGG"


@pytest.fixture(scope="module")
def eng():
    from varkoder_amd.engine import ImageEngine
    e = ImageEngine(k=7, mapping="cgr", device=0)
    yield e
    e.close()


def layout(samples):
    """Files of a batch: (texts, roles, owners) for samples [(r1, r2, singles)]."""
    texts, roles, owner = [], [], []
    for j, (r1, r2, se) in enumerate(samples):
        for recs, role in ((se, _capi.VK_CL_ROLE_UNPAIRED), (r1, _capi.VK_CL_ROLE_R1), (r2, _capi.VK_CL_ROLE_R2)):
            if recs:
                texts.append(R.fq(recs))
                roles.append(role)
                owner.append(j)
    return texts, roles, owner


def mixed_batch():
    """TruSeq pairs whose short inserts the overlap cannot see; single-end Nextera; no adapter; R1 and R2 with
    different adapters (and single reads of their own)."""
    truseq = A.pairs_with_adapters(21, 6000, 0.3)
    nextera = A.se_readthrough(22, 8000, 0.2, adapter=A.NEXTERA)
    plain = R.synth_set(23, 0, 4000, dup_frac=0.0)[2]
    other1, other2 = A.pairs_with_adapters(24, 5000, 0.3, adapter1=A.NEXTERA, adapter2=SMALL_RNA)
    return [(truseq[0], truseq[1], []), ([], [], nextera), ([], [], plain),
            (other1, other2, A.se_readthrough(25, 3000, 0.1))]


def test_detection_equals_reference(eng):
    samples = mixed_batch()
    texts, roles, owner = layout(samples)
    dev, offs, lens = eng.upload(texts)
    records = eng.clean_lines(dev, offs, lens) // 4
    got = eng.detect_adapters(dev, offs, lens, records, roles, owner, len(samples), trim_tail=10)
    want = [A.group_adapters(r1, r2, se, T=10) for r1, r2, se in samples]
    assert got == want
    assert want[0][:2] == [A.TRUSEQ1, A.TRUSEQ2] and want[1][2] == A.NEXTERA and want[2] == [None] * 3
    assert want[3][:3] == [A.NEXTERA, SMALL_RNA, A.TRUSEQ1]


def sliced_batch():
    """12 samples with R1, R2 and single reads each: 36 groups with records, more than the 32 that detection takes per
    slice, so its slice loop runs twice.  The second slice holds sample 10's single reads and sample 11; the adapters
    rotate over the samples, so the groups on either side of the boundary differ."""
    rota = [(A.TRUSEQ1, A.TRUSEQ2, A.NEXTERA), (A.NEXTERA, SMALL_RNA, A.TRUSEQ1), (SMALL_RNA, A.NEXTERA, A.TRUSEQ2)]
    samples = []
    for j in range(12):
        a1, a2, a3 = rota[j % 3]
        r1, r2 = A.pairs_with_adapters(60 + 2 * j, 3000, 0.3, adapter1=a1, adapter2=a2)
        samples.append((r1, r2, A.se_readthrough(61 + 2 * j, 3000, 0.2, adapter=a3)))
    return samples, [list(rota[j % 3]) for j in range(12)]


def test_detection_over_two_slices(eng):
    samples, planted = sliced_batch()
    texts, roles, owner = layout(samples)
    assert len(texts) == 36
    dev, offs, lens = eng.upload(texts)
    records = eng.clean_lines(dev, offs, lens) // 4
    got = eng.detect_adapters(dev, offs, lens, records, roles, owner, len(samples), trim_tail=10)
    want = [A.group_adapters(r1, r2, se, T=10) for r1, r2, se in samples]
    assert got == want
    assert want == planted


def test_detection_unsnapped_and_tail(eng):
    """An unlisted dimer is accepted as its consensus; T changes the forward extension's reach."""
    samples = [([], [], A.dimers(31, 6000, 0.1)), ([], [], A.repeat_reads(32, 6000, 0.2)),
               ([], [], A.se_readthrough(33, 6000, 0.2, adapter=A.UNLISTED))]
    texts, roles, owner = layout(samples)
    dev, offs, lens = eng.upload(texts)
    records = eng.clean_lines(dev, offs, lens) // 4
    for T in (0, 10, 25):
        got = eng.detect_adapters(dev, offs, lens, records, roles, owner, len(samples), trim_tail=T)
        assert got == [A.group_adapters(*s, T=T) for s in samples], T
    assert got[0][2] is not None and got[1][2] is None and got[2][2] is None


def check(samples, texts, st, status, ast, F, T, merge, dedup, table):
    assert not status.any(), status
    for j, (r1, r2, se) in enumerate(samples):
        want, ws, wa = A.clean_sample_adapters(r1, r2, se, F=F, T=T, merge=merge, dedup=dedup, adapters=table[j])
        assert texts[j] == want, f"sample {j}: {len(texts[j])} vs {len(want)} bytes"
        assert int(st[j][0]) == ws["clean_bp"] and int(st[j][1]) == ws["records"]
        assert st[j][2:162].reshape(40, 4).tolist() == ws["base"] and st[j][162:202].tolist() == ws["reach"]
        assert ast[j].tolist() == [wa["reads"], wa["bases"]], j


def run_clean(eng, dev, offs, lens, roles, owner, n, **kw):
    records = eng.clean_lines(dev, offs, lens) // 4
    out, oo, ol, st, status, *rest = eng.clean(dev, offs, lens, records, roles, owner, n, **kw)
    host = out.cpu().numpy()
    return [host[int(oo[j]):int(oo[j]) + int(ol[j])].tobytes() for j in range(n)], st, status, rest


@pytest.mark.parametrize("merge,dedup", [(m, d) for m in (True, False) for d in (True, False)])
@pytest.mark.parametrize("mode", ["explicit", "detect"])
def test_clean_equals_reference(eng, mode, merge, dedup, tmp_path):
    samples = mixed_batch()
    texts, roles, owner = layout(samples)
    if mode == "explicit":
        table = [[A.TRUSEQ1, A.TRUSEQ2, A.TRUSEQ1]] * 2 + [[A.NEXTERA, A.NEXTERA, A.NEXTERA]] * 2
        dev, offs, lens = eng.upload(texts)
    else:   # the product's path: files on disk, some .fq.gz (inflated in HBM)
        paths = []
        for i, t in enumerate(texts):
            p = tmp_path / (f"f{i}.fq.gz" if i % 2 == 0 else f"f{i}.fq")
            p.write_bytes(gzip.compress(t) if i % 2 == 0 else t)
            paths.append(p)
        dev, offs, lens = eng.upload_files(paths)
        records = eng.clean_lines(dev, offs, lens) // 4
        table = eng.detect_adapters(dev, offs, lens, records, roles, owner, len(samples), trim_tail=7)
        assert table == [A.group_adapters(*s, T=7) for s in samples]
    got, st, status, (ast,) = run_clean(eng, dev, offs, lens, roles, owner, len(samples), trim=(5, 7), merge=merge,
                                        dedup=dedup, adapters=table)
    check(samples, got, st, status, ast, 5, 7, merge, dedup, table)


def test_unusual_adapters(eng):
    """Short (4, 7 bases) and long (64) explicit adapters, and a detected-style one holding an N, against reads with
    N bases."""
    r1, r2, se = R.synth_set(41, 3000, 3000)
    n_ad = A.TRUSEQ1[:12] + b"N" + A.TRUSEQ1[13:]
    se = se + [(b"@nn%d" % i, A._rng_seq(np.random.default_rng(i), 40) + n_ad + b"ACGT" * 10, b"I" * (73 + 40))
               for i in range(50)]
    samples = [(r1, r2, se)] * 4
    table = [[b"ACGT", b"AGATCGG", n_ad], [A.TRUSEQ1 + A.TRUSEQ2[:31], None, b"ACGTACGTACGT"],
             [None, A.TRUSEQ2, None], [n_ad, n_ad, A.TRUSEQ1]]
    texts, roles, owner = layout(samples)
    dev, offs, lens = eng.upload(texts)
    got, st, status, (ast,) = run_clean(eng, dev, offs, lens, roles, owner, len(samples), adapters=table)
    check(samples, got, st, status, ast, 10, 10, True, True, table)


def test_without_adapters_unchanged(eng):
    samples = mixed_batch()
    texts, roles, owner = layout(samples)
    dev, offs, lens = eng.upload(texts)
    plain, st0, status0, rest = run_clean(eng, dev, offs, lens, roles, owner, len(samples))
    assert rest == []
    for j, (r1, r2, se) in enumerate(samples):
        assert plain[j] == R.clean_sample(r1, r2, se)[0]
    none, st1, status1, (ast,) = run_clean(eng, dev, offs, lens, roles, owner, len(samples), adapters=[[None] * 3] * 4)
    assert none == plain and (st1 == st0).all() and (status1 == status0).all() and not ast.any()


def run_cli(args, cwd):
    e = dict(os.environ, PYTHONPATH=str(ROOT))
    p = subprocess.run([sys.executable, "-m", "varkoder_amd", "image"] + args, cwd=cwd, env=e, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_cli_detect_adapters_end_to_end(tmp_path):
    se = A.se_readthrough(51, 8000, 0.3)
    d = tmp_path / "raw" / "taxA" / "sampleA"
    d.mkdir(parents=True)
    (d / "sampleA.fq.gz").write_bytes(gzip.compress(R.fq(se)))
    common = ["-R", "7", "-m", "20K", "-M", "300K", "-k", "7"]
    run_cli(["--from-raw", str(tmp_path / "raw"), "-o", "out_plain", "-f", "plain.csv", "-i", "int_plain"] + common,
            tmp_path)
    run_cli(["--from-raw", "--detect-adapters", str(tmp_path / "raw"), "-o", "out_ad", "-f", "ad.csv", "-i", "int_ad"]
            + common, tmp_path)
    report = json.loads((tmp_path / "int_ad" / "clean_reads" / "sampleA_fastp_gpu.json").read_text())
    cut = report["adapter_cutting"]
    assert cut["single_adapter_sequence"] == A.TRUSEQ1.decode()
    assert cut["read1_adapter_sequence"] is None and cut["read2_adapter_sequence"] is None
    _, _, wa = A.clean_sample_adapters([], [], se, adapters=(None, None, A.TRUSEQ1))
    assert [cut["adapter_trimmed_reads"], cut["adapter_trimmed_bases"]] == [wa["reads"], wa["bases"]] and wa["reads"] > 0
    plain = json.loads((tmp_path / "int_plain" / "clean_reads" / "sampleA_fastp_gpu.json").read_text())
    assert "adapter_cutting" not in plain
    text = gzip.decompress((tmp_path / "int_ad" / "clean_reads" / "sampleA.fq.gz").read_bytes())
    seqs = text.split(b"\n")[1::4]
    assert not any(A.TRUSEQ1[i:i + 16] in s for s in seqs for i in range(len(A.TRUSEQ1) - 15))
    before = gzip.decompress((tmp_path / "int_plain" / "clean_reads" / "sampleA.fq.gz").read_bytes())
    assert any(A.TRUSEQ1[:16] in s for s in before.split(b"\n")[1::4])
    a = sorted(p.relative_to(tmp_path / "out_ad") for p in (tmp_path / "out_ad").rglob("*.png"))
    b = sorted(p.relative_to(tmp_path / "out_plain") for p in (tmp_path / "out_plain").rglob("*.png"))
    assert a and a == b
    assert any((tmp_path / "out_ad" / p).read_bytes() != (tmp_path / "out_plain" / p).read_bytes() for p in a)
