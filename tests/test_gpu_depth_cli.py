"""`--depth-filter` end to end.  `image --from-clean --kmer-spectrum D --depth-filter BAND` on two tiny libraries, each a
30x genome (the "organelle") beside a 0.05x one (the "nuclear" part), once with `2:` and once with `:1`: the images are
those of a run WITHOUT the flag on the text that tests/depth_ref.py keeps, stats.csv gains the three columns, and every
`.spectrum.json` holds the spectrum of the text before the filter plus the `"depth_filter"` object.  The same through
`query`.  A band in multiples of the coverage on a sample without an estimate is not applied: `"applied": false`, one
warning line, the images of the unfiltered run."""
import gzip
import json

import numpy as np
import pytest

import depth_ref as D
import spectrum_cases as SC
import spectrum_ref as R
from screen_cases import fq
from test_gpu_query_raw import model_files, query
from test_gpu_spectrum_cli import read_stats
from test_gpu_write_splits import pngs, run
from varkoder_amd import depth
from varkoder_amd import spectrum as S

pytestmark = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "5K", "-M", "20K", "-k", "7"]
NEW = ["depth_reads_in", "depth_reads_removed", "depth_basepairs_removed"]
BANDS = {"2:": (2, D.OPEN), ":1": (0, 1)}


def mixed(seed):
    """6,000 reads of a 20 kb genome (30x) shuffled among 1,000 reads of a 2 Mb genome (0.05x), 100 bases each"""
    rng = np.random.default_rng(seed)
    reads = SC.simulated_reads(rng, 20000, 6000, 100, 0.005) + SC.simulated_reads(rng, 2000000, 1000, 100, 0.005)
    return fq([reads[i] for i in rng.permutation(len(reads))])


def texts():
    return {"libA": mixed(21), "libB": mixed(22)}


def write_clean(folder, samples):
    folder.mkdir(parents=True)
    for s, t in samples.items():
        (folder / f"{s}.fq.gz").write_bytes(gzip.compress(t, compresslevel=1))


def same_pngs(a, b, samples):
    fa, fb = pngs(a), pngs(b)
    assert fa and sorted(fa) == sorted(fb) and {n.split("@")[0] for n in fa} == set(samples)
    for name in fa:
        assert fa[name].read_bytes() == fb[name].read_bytes(), name


@pytest.mark.parametrize("band", sorted(BANDS))
def test_image_from_clean_equals_a_run_on_the_kept_text(tmp_path, band):
    import pandas as pd
    lo, hi = BANDS[band]
    samples = texts()
    ref = {s: D.depth_count(t, 21, 1, lo, hi) for s, t in samples.items()}
    assert all(0 < r[1][D.KEPT] < r[1][D.IN] for r in ref.values())
    write_clean(tmp_path / "int" / "clean_reads", samples)
    write_clean(tmp_path / "kept" / "clean_reads", {s: r[0] for s, r in ref.items()})
    run(["--from-clean", "int", "-o", "img1", "-f", "s1.csv", "--kmer-spectrum", "spec", "--depth-filter", band] + COMMON, tmp_path)
    run(["--from-clean", "kept", "-o", "img0", "-f", "s0.csv"] + COMMON, tmp_path)
    same_pngs(tmp_path / "img0", tmp_path / "img1", samples)
    s0, s1 = read_stats(tmp_path / "s0.csv"), read_stats(tmp_path / "s1.csv")
    assert [c for c in s1.columns if c in NEW] == NEW
    keep = [c for c in s0.columns if not c.endswith("_time")]
    pd.testing.assert_frame_equal(s0[keep], s1[keep], check_exact=True)
    for s, t in samples.items():
        row = ref[s][1]
        for name, v in depth.columns(row).items():
            assert int(s1.loc[s, name]) == v, (s, name)
        assert int(s1.loc[s, "depth_reads_removed"]) == int(row[D.IN] - row[D.KEPT]) > 0
        got = json.loads((tmp_path / "spec" / f"{s}.spectrum.json").read_text())
        dp = got.pop("depth_filter")
        assert dp == json.loads(json.dumps(depth.report(row, depth.parse_band(band), (lo, hi), True, None)))
        assert dp["applied"] is True and dp["band"] == band and sum(dp["median_depth_histogram"]) + dp["median_depth_255_and_more"] == dp["reads_in"]
        # the spectrum describes the text before the filter
        assert got == json.loads(json.dumps(S.report(R.spectrum_numpy(t, 21, 1)[0], 21, 1)))
        # bimodal: reads at depth 0..2 and reads around the organelle's coverage, little between
        h = dp["median_depth_histogram"]
        assert sum(h[:3]) > 500 and sum(h[10:]) > 4000 and sum(h[4:8]) < 100


@pytest.mark.parametrize("band", sorted(BANDS))
def test_query_equals_a_run_on_the_kept_text(tmp_path, band):
    lo, hi = BANDS[band]
    samples = texts()
    ref = {s: D.depth_count(t, 21, 1, lo, hi) for s, t in samples.items()}
    write_clean(tmp_path / "clean", samples)
    write_clean(tmp_path / "kept", {s: r[0] for s, r in ref.items()})
    model_files(tmp_path)
    common = ["-R", "5", "-M", "20K", "-b", "2", "-P"]
    query(tmp_path, tmp_path / "clean", tmp_path / "out1", "--kmer-spectrum", tmp_path / "spec", "--depth-filter", band, *common)
    query(tmp_path, tmp_path / "kept", tmp_path / "out0", *common)
    a, b = ((tmp_path / d / "predictions.csv").read_text().replace(str(tmp_path / d), "") for d in ("out1", "out0"))
    assert a == b and a.count("\n") == 3
    for s in samples:
        dp = json.loads((tmp_path / "spec" / f"{s}.spectrum.json").read_text())["depth_filter"]
        assert dp == json.loads(json.dumps(depth.report(ref[s][1], depth.parse_band(band), (lo, hi), True, None)))


def test_a_band_in_multiples_of_the_coverage(tmp_path, capsys):
    """`0.5x:` -- the deep sample is filtered at ceil(0.5 lambda); the shallow one has no estimate: not applied, one
    warning line, the images of the unfiltered run"""
    rng = np.random.default_rng(23)
    samples = {"deep": mixed(24), "shallow": fq(SC.simulated_reads(rng, 2000000, 400, 100, 0.005))}
    est = S.estimate(R.spectrum_numpy(samples["deep"], 21, 1)[0], 21, 1)
    band = depth.parse_band("0.5x:")
    lo, hi, applied, _ = depth.resolve(band, est)
    assert applied and 5 <= lo <= 20 and hi == D.OPEN
    ref = D.depth_count(samples["deep"], 21, 1, lo, hi)
    write_clean(tmp_path / "int" / "clean_reads", samples)
    write_clean(tmp_path / "kept" / "clean_reads", {"deep": ref[0], "shallow": samples["shallow"]})
    capsys.readouterr()
    run(["--from-clean", "int", "-o", "img1", "-f", "s1.csv", "--kmer-spectrum", "spec", "--depth-filter", "0.5x:"] + COMMON, tmp_path)
    err = capsys.readouterr().err
    assert err.count("DEPTH FILTER SKIPPED:") == 1 and "too few repeated k-mers" in err
    run(["--from-clean", "kept", "-o", "img0", "-f", "s0.csv"] + COMMON, tmp_path)
    same_pngs(tmp_path / "img0", tmp_path / "img1", samples)
    deep, shallow = (json.loads((tmp_path / "spec" / f"{s}.spectrum.json").read_text())["depth_filter"] for s in ("deep", "shallow"))
    assert deep == json.loads(json.dumps(depth.report(ref[1], band, (lo, hi), True, None))) and deep["lo"] == lo
    assert shallow["applied"] is False and "too few repeated k-mers" in shallow["reason"] and shallow["band"] == "0.5x:"
    assert (shallow["lo"], shallow["hi"]) == (0, None) and shallow["reads_kept"] == shallow["reads_in"] == 400
    assert sum(shallow["median_depth_histogram"]) == 400   # (its histogram is still counted)
    s1 = read_stats(tmp_path / "s1.csv")
    assert int(s1.loc["shallow", "depth_reads_removed"]) == 0 < int(s1.loc["deep", "depth_reads_removed"])


def test_image_from_raw_files_qc_and_images_see_what_is_kept(tmp_path):
    """clean -> spectrum -> depth filter -> qc-after -> ladder: the clean_reads files hold what the rule keeps of the
    cleaned text, the QC's after section counts those reads, the images are those of the kept text"""
    from test_gpu_spectrum_cli import SETS, write_raw
    write_raw(tmp_path / "raw", nested=True)
    run(["--from-raw", "raw", "-i", "int0", "-o", "img0", "-f", "s0.csv"] + COMMON, tmp_path)
    cleaned = {s: gzip.decompress((tmp_path / "int0" / "clean_reads" / f"{s}.fq.gz").read_bytes()) for s in SETS}
    ref = {s: D.depth_count(t, 16, 1, 0, 1) for s, t in cleaned.items()}
    assert any(0 < r[1][D.KEPT] < r[1][D.IN] for r in ref.values())
    run(["--from-raw", "raw", "-i", "int1", "-o", "img1", "-f", "s1.csv", "--kmer-spectrum", "spec", "--spectrum-k", "16",
         "--depth-filter", ":1", "--qc-report", "qc"] + COMMON, tmp_path)
    stats = read_stats(tmp_path / "s1.csv")
    for s in SETS:
        assert gzip.decompress((tmp_path / "int1" / "clean_reads" / f"{s}.fq.gz").read_bytes()) == ref[s][0]
        qc = json.loads((tmp_path / "qc" / f"{s}.qc.json").read_text())
        assert qc["summary"]["after_filtering"]["total_reads"] == int(ref[s][1][D.KEPT]) == int(stats.loc[s, "clean_reads"])
        assert int(stats.loc[s, "depth_reads_in"]) == int(ref[s][1][D.IN])
        got = json.loads((tmp_path / "spec" / f"{s}.spectrum.json").read_text())
        assert got["reads"] == int(ref[s][1][D.IN]) and got["depth_filter"]["reads_kept"] == int(ref[s][1][D.KEPT])
    # the images: the pixels of a run from the files the filtered run left, without the flag (the two entries word a
    # text chunk differently, so the files' bytes are not compared)
    from PIL import Image
    run(["--from-clean", "int1", "-o", "img2", "-f", "s2.csv"] + COMMON, tmp_path)
    fa, fb = pngs(tmp_path / "img2"), pngs(tmp_path / "img1")
    assert fa and sorted(fa) == sorted(fb) and {n.split("@")[0] for n in fa} == set(SETS)
    for name in fa:
        assert np.array_equal(np.array(Image.open(fa[name])), np.array(Image.open(fb[name]))), name
