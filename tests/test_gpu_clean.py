"""Step B on the MI355X (vk_clean_device through ImageEngine.clean): the cleaned FASTQ bytes and the stats equal
tests/clean_ref.py's on the hand cases, on seeded synthetic sets (plain and .fq.gz, every -a/-D/-r combination), with
a dedup hash narrowed to a few bits; bad input gives a status; `image --from-raw` end to end."""
import gzip
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_ref as R  # noqa: E402

from varkoder_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FLAGS = [(a, m, d) for a in (True, False) for m in (True, False) for d in (True, False)]


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


def gpu_clean(eng, dev, offs, lens, roles, owner, n, records=None, **kw):
    if records is None:
        records = eng.clean_lines(dev, offs, lens) // 4
    out, oo, ol, st, status = eng.clean(dev, offs, lens, records, roles, owner, n, **kw)
    host = out.cpu().numpy()
    return [host[int(oo[j]):int(oo[j]) + int(ol[j])].tobytes() for j in range(n)], st, status


def check(samples, texts, st, status, F, T, adapter, merge, dedup):
    assert not status.any(), status
    for j, (r1, r2, se) in enumerate(samples):
        want, ws = R.clean_sample(r1, r2, se, F=F, T=T, adapter=adapter, merge=merge, dedup=dedup)
        assert texts[j] == want, f"sample {j}: {len(texts[j])} vs {len(want)} bytes"
        assert int(st[j][0]) == ws["clean_bp"] and int(st[j][1]) == ws["records"]
        assert st[j][2:162].reshape(40, 4).tolist() == ws["base"] and st[j][162:202].tolist() == ws["reach"]


@pytest.mark.parametrize("adapter,merge,dedup", FLAGS)
def test_hand_cases(eng, adapter, merge, dedup):
    cases = R.hand_cases()
    for FT in sorted({(c["F"], c["T"]) for c in cases.values()}):
        samples = [(c["r1"], c["r2"], c["singles"]) for c in cases.values() if (c["F"], c["T"]) == FT]
        texts, roles, owner = layout(samples)
        dev, offs, lens = eng.upload(texts)
        got, st, status = gpu_clean(eng, dev, offs, lens, roles, owner, len(samples), trim=FT, adapter=adapter,
                                    merge=merge, dedup=dedup)
        check(samples, got, st, status, FT[0], FT[1], adapter, merge, dedup)


def test_synthetic_100k_pairs(eng):
    samples = [R.synth_set(101, 100000, 20000), R.synth_set(102, 0, 5000), R.synth_set(103, 3000, 0)]
    texts, roles, owner = layout(samples)
    dev, offs, lens = eng.upload(texts)
    got, st, status = gpu_clean(eng, dev, offs, lens, roles, owner, len(samples))
    check(samples, got, st, status, 10, 10, True, True, True)


@pytest.mark.parametrize("adapter,merge,dedup", FLAGS[1:])
def test_synthetic_flag_combinations(eng, adapter, merge, dedup):
    samples = [R.synth_set(200 + len(FLAGS), 8000, 2000, L=101)]
    texts, roles, owner = layout(samples)
    dev, offs, lens = eng.upload(texts)
    got, st, status = gpu_clean(eng, dev, offs, lens, roles, owner, 1, trim=(5, 3), adapter=adapter, merge=merge,
                                dedup=dedup)
    check(samples, got, st, status, 5, 3, adapter, merge, dedup)


def test_gz_and_plain_files_on_disk(eng, tmp_path):
    """Files read through the product's path (upload_files: a .fq.gz is inflated in HBM), two samples, several files
    per group (records concatenate in file order)."""
    r1, r2, se = R.synth_set(7, 6000, 3000)
    paths, roles, owner = [], [], []
    for name, recs, role, gz in (("a_R1.fq.gz", r1[:4000], 1, True), ("b_R1.fq", r1[4000:], 1, False),
                                 ("a_R2.fq.gz", r2[:2500], 2, True), ("b_R2.fq.gz", r2[2500:], 2, True),
                                 ("s.fq.gz", se, 0, True)):
        p = tmp_path / name
        p.write_bytes(gzip.compress(R.fq(recs)) if gz else R.fq(recs))
        paths.append(p)
        roles.append(role)
        owner.append(0)
    p = tmp_path / "other.fq"
    p.write_bytes(R.fq(se[:500]))
    paths.append(p)
    roles.append(0)
    owner.append(1)
    dev, offs, lens = eng.upload_files(paths)
    got, st, status = gpu_clean(eng, dev, offs, lens, roles, owner, 2)
    check([(r1, r2, se), ([], [], se[:500])], got, st, status, 10, 10, True, True, True)


def test_narrow_hash_is_still_exact(monkeypatch):
    """VKIMG_CLEAN_HASH_BITS=3: every read shares its hash with an eighth of the others; the byte comparison keeps the
    dedup exact."""
    from varkoder_amd.engine import ImageEngine
    monkeypatch.setenv("VKIMG_CLEAN_HASH_BITS", "3")
    e = ImageEngine(k=7, mapping="cgr", device=0)
    try:
        samples = [R.synth_set(31, 3000, 1500, dup_frac=0.3), R.synth_set(32, 500, 500, dup_frac=0.3)]
        texts, roles, owner = layout(samples)
        dev, offs, lens = e.upload(texts)
        got, st, status = gpu_clean(e, dev, offs, lens, roles, owner, 2)
        check(samples, got, st, status, 10, 10, True, True, True)
    finally:
        e.close()


def test_bad_input_gives_a_status(eng):
    good = R.synth_set(41, 50, 20)
    r1, r2, se = R.synth_set(42, 30, 10)
    texts, roles, owner = layout([good])
    texts += [R.fq(r1), R.fq(r2[:29])]                                    # 1: ragged pair (30 against 29 records)
    roles += [1, 2]
    owner += [1, 1]
    texts += [R.fq(se).replace(b"@s3\n", b"s3@\n", 1)]                   # 2: a header without '@'
    roles += [0]
    owner += [2]
    texts += [R.fq(se).replace(b"\n+\n", b"\n-\n", 1)]                   # 3: third line not '+'
    roles += [0]
    owner += [3]
    bad_q = R.fq(se[:3]) + b"@q\nACGT\n+\nIII\n"                         # 4: quality shorter than the sequence
    texts += [bad_q]
    roles += [0]
    owner += [4]
    texts += [R.fq(se)]                                                   # 5: a budget past the file's records
    roles += [0]
    owner += [5]
    dev, offs, lens = eng.upload(texts)
    records = eng.clean_lines(dev, offs, lens) // 4
    records[-1] += 1
    got, st, status = gpu_clean(eng, dev, offs, lens, roles, owner, 6, records=records)
    assert status.tolist() == [0, _capi.VK_CL_RAGGED] + [_capi.VK_CL_BAD_FRAMING] * 4
    assert got[0] == R.clean_sample(*good)[0]
    assert all(t == b"" for t in got[1:])


def run_cli(args, cwd, env=None):
    e = dict(os.environ, PYTHONPATH=str(ROOT), **(env or {}))
    p = subprocess.run([sys.executable, "-m", "varkoder_amd", "image"] + args, cwd=cwd, env=e, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_cli_from_raw_end_to_end(tmp_path):
    """`image --from-raw` on a <taxon>/<sample>/ tree (a paired sample as .fq.gz, a single-end one as plain text, a
    sample with both) writes the PNGs `image --from-clean` writes from clean_ref's output with the same seed."""
    import pandas as pd
    raw = tmp_path / "raw"
    plan = {("taxA", "sampleA"): R.synth_set(51, 3000, 0), ("taxB", "sampleB"): R.synth_set(52, 0, 5000),
            ("taxB", "sampleC"): R.synth_set(53, 2000, 1500)}
    clean = tmp_path / "clean"
    clean.mkdir()
    for (taxon, sample), (r1, r2, se) in plan.items():
        d = raw / taxon / sample
        d.mkdir(parents=True)
        if r1:
            (d / f"{sample}_R1.fq.gz").write_bytes(gzip.compress(R.fq(r1)))
            (d / f"{sample}_R2.fq.gz").write_bytes(gzip.compress(R.fq(r2)))
        if se:
            (d / f"{sample}_se.fq").write_bytes(R.fq(se))
        text, st = R.clean_sample(r1, r2, se)
        (clean / f"{sample}.fq").write_bytes(text)
        from varkoder_amd.rawinput import content_curves
        import json
        (clean / f"{sample}_fastp_gpu.json").write_text(json.dumps(
            {"read1_after_filtering": {"content_curves": content_curves(st["base"], st["reach"])}}))
    pd.DataFrame({"sample": [s for _, s in plan], "labels": [t for t, _ in plan]}).to_csv(tmp_path / "labels.csv", index=False)
    common = ["-R", "7", "-m", "20K", "-M", "300K", "-k", "7", "-t"]
    run_cli(["--from-raw", str(raw), "-o", "out_raw", "-f", "raw.csv", "-i", "int"] + common, tmp_path)
    run_cli(["--from-clean", str(clean), "-o", "out_clean", "-f", "clean.csv", "--labels-csv", "labels.csv"] + common,
            tmp_path)
    a = sorted(p.relative_to(tmp_path / "out_raw") for p in (tmp_path / "out_raw").rglob("*.png"))
    b = sorted(p.relative_to(tmp_path / "out_clean") for p in (tmp_path / "out_clean").rglob("*.png"))
    assert a and a == b and len({p.name.split("@")[0] for p in a}) == 3
    for p in a:
        assert (tmp_path / "out_raw" / p).read_bytes() == (tmp_path / "out_clean" / p).read_bytes(), p
    stats = pd.read_csv(tmp_path / "raw.csv").set_index("sample")
    for (taxon, sample), (r1, r2, se) in plan.items():
        _, st = R.clean_sample(r1, r2, se)
        assert stats.loc[sample, "clean_basepairs"] == st["clean_bp"]
        assert stats.loc[sample, "cleaning_time"] > 0
        assert stats.loc[sample, "base_frequencies_sd"] > 0
        assert gzip.decompress((tmp_path / "int" / "clean_reads" / f"{sample}.fq.gz").read_bytes()) == \
            (clean / f"{sample}.fq").read_bytes()
    labels = pd.read_csv(tmp_path / "out_raw" / "labels.csv").set_index("sample")
    assert labels.loc["sampleA", "labels"] == "taxA" and labels.loc["sampleC", "labels"] == "taxB"
    # a second run finds the cleaned files and takes them as they are
    p = run_cli(["--from-raw", str(raw), "-o", "out_again", "-f", "again.csv", "-i", "int"] + common, tmp_path)
    assert "Skipping cleaning for sampleA: File exists." in p.stderr
    again = sorted(q.relative_to(tmp_path / "out_again") for q in (tmp_path / "out_again").rglob("*.png"))
    assert again == a
    for q in a:
        assert (tmp_path / "out_again" / q).read_bytes() == (tmp_path / "out_raw" / q).read_bytes(), q
