"""`--from-fasta --per-record` on the GPU: vk_fasta_records_count_device, vk_fasta_records_device and
vk_count_fasta_records_device against tests/fasta_records_ref.py (record counts, starts, bases, names and every selected
record's histogram equal, k = 5..9), with VKIMG_FASTA_UNIT_BYTES small in one engine and at its default in another; then
the commands.  Expected rows are kept sparse and compared on the device."""
import functools
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_records_cases as RC  # noqa: E402
import fasta_records_ref as RR  # noqa: E402
import fasta_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu
KS = FC.KS
UNITS = ("small", "default")
GROUPS = {"seams_small": RC.seam_cases_small, "seams_default": RC.seam_cases_default, "many": RC.many_cases,
          "long": RC.long_cases, "carry": RC.carry_case, "slots": RC.slot_batch, "batch": RC.batch_cases}


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
def cases_of(group):
    return GROUPS[group]()


@functools.lru_cache(maxsize=None)
def expected_table(group):
    """Per sample (status, [(start, bases, kept name)]): computed once, shared by every k, left unchanged."""
    return [(FR.status(d), RR.table(d)) for _, d in cases_of(group)]


@functools.lru_cache(maxsize=None)
def expected_rows(group, k):
    """Per sample, per record: the non-zero bins of its histogram (codes, counts)."""
    out = []
    for _, d in cases_of(group):
        rows = []
        for r in RR.joined(d):
            h = RR.count(r, k)
            nz = np.flatnonzero(h)
            rows.append((nz, h[nz].astype(np.int64)))
        out.append(rows)
    return out


def table_of(eng, group):
    data = [d for _, d in cases_of(group)]
    dev, offs, lens = eng.upload(data)
    return (dev, offs, lens), eng.fasta_records(dev, offs, lens)


def check_table(group, tab):
    rec_first, start, bases, names, status = tab
    want = expected_table(group)
    assert len(rec_first) == len(want) + 1 and rec_first[0] == 0
    for i, ((name, _), (ws, wt)) in enumerate(zip(cases_of(group), want)):
        a, b = int(rec_first[i]), int(rec_first[i + 1])
        assert int(status[i]) == ws, name
        assert b - a == len(wt), name
        got = [(int(start[g]), int(bases[g]), names[g].ljust(RR.NAME_BYTES, b"\0")) for g in range(a, b)]
        assert got == wt, name


def assert_rows(hist, want):
    """hist [nslots, 4^k] on the device equals want = {slot: (codes, counts)}; every other row is zero."""
    import torch
    exp = torch.zeros_like(hist)
    for sl, (codes, counts) in want.items():
        if len(codes):
            exp[sl, torch.from_numpy(codes).to(hist.device)] = torch.from_numpy(counts.astype(np.uint32).view(np.int32)).to(hist.device)
    if not torch.equal(hist, exp):
        bad = (hist != exp).any(dim=1).nonzero().flatten().tolist()
        raise AssertionError(f"rows differ: {bad[:10]} ({len(bad)} of {hist.shape[0]})")


def check_count(eng, group, k, buf, tab, select=lambda s, r, g: True, spare=0):
    """One call over the group's batch with a slot for every record that `select(sample, ordinal, g)` takes."""
    rec_first = tab[0]
    total = int(rec_first[-1])
    slot = np.full(total, RR.NO_SLOT, dtype=np.uint32)
    want, n = {}, 0
    for s, rows in enumerate(expected_rows(group, k)):
        for r, row in enumerate(rows):
            g = int(rec_first[s]) + r
            if select(s, r, g):
                slot[g] = n
                want[n] = row
                n += 1
    hist = eng.count_fasta_records(*buf, rec_first, slot, max(n + spare, 1))
    assert_rows(hist, want)
    return hist, slot


def check_invariants(eng, buf, tab, hist):
    """With every record selected: the rows and the bases of a sample's records sum to count_fasta's."""
    rec_first, _, bases = tab[:3]
    whole, status, wbases = eng.count_fasta(*buf)
    wbases = wbases.cpu().numpy()
    for s in range(len(rec_first) - 1):
        a, b = int(rec_first[s]), int(rec_first[s + 1])
        if int(status[s]):
            assert a == b
            continue
        assert int(bases[a:b].sum()) == int(wbases[s])
        got = (hist[a:b].long().sum(dim=0) & 0xFFFFFFFF) if b > a else 0
        assert bool(((whole[s].long() & 0xFFFFFFFF) == got).all()), s


def check_group(eng, group, k):
    buf, tab = table_of(eng, group)
    check_table(group, tab)
    hist, _ = check_count(eng, group, k, buf, tab)
    check_invariants(eng, buf, tab, hist)


@pytest.mark.parametrize("k", KS)
def test_seams_small_unit(fa_engines, k):
    """A second header moved in steps of one over every lane seam of two units of 256 bytes and over the unit seams; its
    name and the line end before it cross them as well.  Table, rows and the sums equal the reference."""
    check_group(fa_engines(k, "small"), "seams_small", k)


@pytest.mark.parametrize("k", KS)
def test_seams_default_unit(fa_engines, k):
    """The same around a wave seam, a unit seam and the seam between two workgroups' spans at the default unit."""
    check_group(fa_engines(k, "default"), "seams_default", k)


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
def test_many_records_per_lane(fa_engines, k, unit):
    """`>\\n`, `>a\\nA\\n`, records of k - 1 and k bases, 32 empty records in 64 bytes, names of 127, 128 and 129 bytes and
    one across a unit seam, a header that is the sample's last line without \\n."""
    check_group(fa_engines(k, unit), "many", k)


@pytest.mark.parametrize("k", KS)
def test_one_record_over_many_spans(fa_engines, k):
    """2 MB in one record at the default unit (k <= 7: every workgroup of it on its LDS table), 300 short records behind
    it; the same file wrapped at 60 columns with CRLF."""
    check_group(fa_engines(k, "default"), "long", k)


@pytest.mark.parametrize("k", KS)
def test_more_units_than_scan_threads(fa_engines, k):
    """100 KB of 40-base records at unit 256: 400 units, the ordinal's carry crosses passes of the scan.  Every eighth
    record has a slot; the table is checked for all."""
    eng = fa_engines(k, "small")
    buf, tab = table_of(eng, "carry")
    check_table("carry", tab)
    assert int(tab[0][-1]) == 2200
    check_count(eng, "carry", k, buf, tab, select=lambda s, r, g: r % 8 == 3)


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
def test_slots(fa_engines, k, unit):
    """Every second record unselected; the entering record of a span unselected; only the last record selected; spare
    slots come back zero; one call equals the calls record_plan cuts with a budget of three rows."""
    import torch
    from varkoder_amd.fasta import record_plan
    eng = fa_engines(k, unit)
    buf, tab = table_of(eng, "slots")
    total = int(tab[0][-1])
    check_count(eng, "slots", k, buf, tab, select=lambda s, r, g: g % 2 == 1)
    check_count(eng, "slots", k, buf, tab, select=lambda s, r, g: r != 0, spare=3)   # (unit 256: records that enter spans)
    check_count(eng, "slots", k, buf, tab, select=lambda s, r, g: g == total - 1)
    whole, _ = check_count(eng, "slots", k, buf, tab)
    calls = record_plan(tab[2], 0, 3 * 4 * eng.ncode, eng.ncode)
    assert [g for c in calls for g in c] == list(range(total)) and max(len(c) for c in calls) == 3
    for c in calls:
        slot = np.full(total, RR.NO_SLOT, dtype=np.uint32)
        slot[c] = np.arange(len(c), dtype=np.uint32)
        part = eng.count_fasta_records(*buf, tab[0], slot, len(c))
        assert torch.equal(part, whole[c[0]:c[-1] + 1])


@pytest.mark.parametrize("k", KS)
def test_entering_record_of_a_default_span_unselected(fa_engines, k):
    """At the default unit the 2 MB record enters every span but the first: without a slot, its workgroups skip their
    text and the 300 records behind it still come out exact; and the reverse, the long record alone."""
    eng = fa_engines(k, "default")
    buf, tab = table_of(eng, "long")
    check_count(eng, "long", k, buf, tab, select=lambda s, r, g: r != 0)
    check_count(eng, "long", k, buf, tab, select=lambda s, r, g: r == 0, spare=2)


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
def test_batch(fa_engines, k, unit):
    """64 samples at every 16-byte residue, with an empty one, a FASTQ (VK_ST_BAD_START, nrec = 0) and a header-only file
    among exact neighbours."""
    eng = fa_engines(k, unit)
    buf, tab = table_of(eng, "batch")
    rec_first, status = tab[0], tab[4]
    names = [n for n, _ in cases_of("batch")]
    for nm, nrec, st in (("batch_empty", 0, 0), ("batch_fastq", 0, 1), ("batch_header_only", 1, 0), ("batch_three", 3, 0)):
        i = names.index(nm)
        assert int(rec_first[i + 1] - rec_first[i]) == nrec and int(status[i]) == st
    check_table("batch", tab)
    hist, _ = check_count(eng, "batch", k, buf, tab)
    check_invariants(eng, buf, tab, hist)


def test_refusals(fa_engines):
    """VK_EINVAL before any launch: null pointers, k outside 5..9, no slots, a rec_first that does not start at 0 or
    decreases."""
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import _u64
    eng = fa_engines(7, "small")
    dev, offs, lens = eng.upload([b">a\nACGTACGTACGT\n>b\nACGTACGTAA\n", b">c\nACGTTTGACA\n"])
    offs, lens = eng._desc(offs, lens)
    good = np.array([0, 2, 3], dtype=np.uint64)
    slot = torch.arange(3, dtype=torch.int32, device=eng.device)
    hist = torch.zeros((3, eng.ncode), dtype=torch.int32, device=eng.device)
    tabs = [torch.zeros(3 * n, dtype=torch.int64, device=eng.device) for n in (1, 1, 16)]

    def count(k=7, rec_first=good, d_slot=slot, nslots=3, d_hist=hist, text=dev):
        return eng.L.vk_count_fasta_records_device(eng.ctx, eng._ptr(text) if text is not None else None, _u64(offs), _u64(lens), 2,
                                                   k, _u64(rec_first) if rec_first is not None else None,
                                                   eng._ptr(d_slot) if d_slot is not None else None, nslots,
                                                   eng._ptr(d_hist) if d_hist is not None else None)

    def table(rec_first=good, which=None):
        ptrs = [None if which == j else eng._ptr(t) for j, t in enumerate(tabs)]
        return eng.L.vk_fasta_records_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), 2,
                                             _u64(rec_first) if rec_first is not None else None, *ptrs)
    assert count() == _capi.VK_OK and table() == _capi.VK_OK
    for kw in (dict(k=4), dict(k=10), dict(nslots=0), dict(rec_first=None), dict(d_slot=None), dict(d_hist=None), dict(text=None),
               dict(rec_first=np.array([1, 2, 3], dtype=np.uint64)), dict(rec_first=np.array([0, 2, 1], dtype=np.uint64))):
        assert count(**kw) == _capi.VK_EINVAL, kw
    for kw in (dict(rec_first=None), dict(which=0), dict(which=1), dict(which=2), dict(rec_first=np.array([1, 2, 3], dtype=np.uint64)),
               dict(rec_first=np.array([0, 2, 1], dtype=np.uint64))):
        assert table(**kw) == _capi.VK_EINVAL, kw
    nrec = torch.zeros(2, dtype=torch.int32, device=eng.device)
    assert eng.L.vk_fasta_records_count_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), 2, None, eng._ptr(nrec)) == _capi.VK_EINVAL
    assert eng.L.vk_fasta_records_count_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), 2, eng._ptr(nrec), None) == _capi.VK_EINVAL


# ---- whole commands -------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MAPPING = 7, "cgr"


def command_files(root):
    """A collection file (two good records, one too short, one with the first one's id, one all N) and a gzipped
    assembly (CRLF, 60 columns); beside it the folder that holds every record to be imaged as a file of its own.
    Returns (folder, folder of single records, {record sample: joined bytes} of the records to be imaged)."""
    src, single = root / "fasta", root / "single"
    src.mkdir()
    single.mkdir()
    coll = [(b"NC_1.1 Homo sapiens mitochondrion", FC.seq(801, 3000)), (b"ctg/2\tlen=1500", FC.seq(802, 1500, b"ACGTacgtN")),
            (b"tiny", FC.seq(803, 200)), (b"NC_1.1 again", FC.seq(804, 1200)), (b"allN", b"N" * 1100)]
    asm = [(b"scaffold_%d cov=%d" % (i, 10 + i), FC.seq(810 + i, 1000 + 450 * i)) for i in range(3)]
    (src / "coll.fa").write_bytes(FC.fasta(coll, 70))
    (src / "asm.fna.gz").write_bytes(gzip.compress(FC.fasta(asm, 60, b"\r\n")))
    (src / "notes.txt").write_bytes(b"not a sample\n")
    good = {"coll__NC_1.1": coll[0][1], "coll__ctg_2": coll[1][1]}
    good.update({"asm__scaffold_%d" % i: s for i, (_, s) in enumerate(asm)})
    for name, s in good.items():
        (single / (name + ".fa")).write_bytes(b">x\n" + FC.wrap(s, 80))
    return src, single, good


def command(*args):
    import subprocess
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "varkoder_amd"] + [str(a) for a in args], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def png_name(sample, nbases):
    return f"{sample}@{str(nbases // 1000).rjust(8, '0')}K+{MAPPING}+k{K}.png"


def test_image_per_record_command(tmp_path):
    import pandas as pd
    from PIL import Image
    from oracle import oracle
    src, single, good = command_files(tmp_path)
    (tmp_path / "labels.csv").write_text("sample,labels\ncoll,family:Hominidae\ncoll__ctg_2,genus:Pan\n")
    out, ref, plain = tmp_path / "images", tmp_path / "images_single", tmp_path / "images_plain"
    err = command("image", src, "--from-fasta", "--per-record", "-k", K, "-p", MAPPING, "-o", out, "-f", tmp_path / "stats.csv",
                  "-t", "--labels-csv", tmp_path / "labels.csv")
    command("image", single, "--from-fasta", "-k", K, "-p", MAPPING, "-o", ref, "-f", tmp_path / "stats_single.csv")
    names = {s: png_name(s, len(b)) for s, b in good.items()}
    assert sorted(p.name for p in out.glob("*.png")) == sorted(names.values())
    for s, name in names.items():   # the pixels of the same record given as a file of its own
        assert np.array_equal(np.array(Image.open(out / name)), np.array(Image.open(ref / name))), s
    assert Image.open(out / names["coll__NC_1.1"]).info["varkoderKeywords"] == "family:Hominidae"
    assert Image.open(out / names["coll__ctg_2"]).info["varkoderKeywords"] == "genus:Pan"
    assert Image.open(out / names["asm__scaffold_1"]).info["varkoderKeywords"] == ""
    stats = pd.read_csv(tmp_path / "stats.csv").set_index("sample")
    assert sorted(stats.index) == sorted(list(good) + ["coll__NC_1.1#4", "coll__allN"])
    for s in good:
        assert stats.loc[s, f"{K}mer_counting_time"] > 0 and stats.loc[s, f"k{K}_img_time"] > 0 and pd.isna(stats.loc[s, "failed_step"])
    assert stats.loc["coll__NC_1.1#4", "failed_step"] == "image" and stats.loc["coll__allN", "failed_step"] == "image"
    assert "DUPLICATE RECORD ID, SKIPPING: coll__NC_1.1" in err
    assert "1 of 5 records shorter than 1000 bases passed over" in err
    lt = pd.read_csv(out / "labels.csv", dtype=str).fillna("").set_index("sample")
    assert sorted(lt.index) == sorted(good)
    assert lt.loc["coll__NC_1.1", "labels"] == "family:Hominidae" and lt.loc["coll__ctg_2", "labels"] == "genus:Pan"
    # --min-record-length takes the short record in, and nothing else changes
    command("image", src, "--from-fasta", "--per-record", "--min-record-length", 200, "-k", K, "-p", MAPPING, "-o", tmp_path / "images200",
            "-f", tmp_path / "stats200.csv")
    assert sorted(p.name for p in (tmp_path / "images200").glob("*.png")) == sorted(list(names.values()) + [png_name("coll__tiny", 200)])
    # without the flag: one image per file, the pixels the oracle gives for the file's records
    command("image", src, "--from-fasta", "-k", K, "-p", MAPPING, "-o", plain, "-f", tmp_path / "stats_plain.csv")
    want = {}
    for f, s in ((src / "coll.fa", "coll"), (src / "asm.fna.gz", "asm")):
        data = gzip.decompress(f.read_bytes()) if f.suffix == ".gz" else f.read_bytes()
        img, _, st = oracle.fastq_to_image(FR.to_fastq(data), K, oracle.cgr_lut(K), 4 ** K)
        assert st == 0
        want[png_name(s, FR.bases(data))] = img
    assert sorted(p.name for p in plain.glob("*.png")) == sorted(want)
    for name, img in want.items():
        assert np.array_equal(np.array(Image.open(plain / name)).ravel(), img), name
    assert sorted(pd.read_csv(tmp_path / "stats_plain.csv")["sample"]) == ["asm", "coll"]


def test_query_per_record_command(tmp_path):
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
    src, single, good = command_files(tmp_path)
    model = ["-l", tmp_path / "m.pt", "--vocab", tmp_path / "vocab.txt", "-k", K, "-p", MAPPING, "-P", "-b", 2]
    command("query", *model, src, tmp_path / "out", "--from-fasta", "--per-record")
    command("query", *model, single, tmp_path / "out_single", "--from-fasta")
    a = pd.read_csv(tmp_path / "out" / "predictions.csv", float_precision="round_trip")
    b = pd.read_csv(tmp_path / "out_single" / "predictions.csv", float_precision="round_trip")
    # a row per record, files in order and records in order within each; each equals the record's row as its own file
    assert list(a["sample_id"]) == ["asm__scaffold_0", "asm__scaffold_1", "asm__scaffold_2", "coll__NC_1.1", "coll__ctg_2"]
    assert list(a["query_basepairs"]) == [len(good[s]) // 1000 * 1000 for s in a["sample_id"]]
    pd.testing.assert_frame_equal(a.sort_values("sample_id").reset_index(drop=True), b.sort_values("sample_id").reset_index(drop=True),
                                  check_exact=True)
