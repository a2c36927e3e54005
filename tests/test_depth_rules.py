"""`--depth-filter` without a GPU: the two statements of the rule (tests/depth_ref.py) held to each other on every case of
tests/depth_cases.py and to what the cases are FOR; varkoder_amd/depth.py -- parse_band, resolve with its ceil and floor,
a sample without an estimate, report and columns; the command line's refusals."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as DC  # noqa: E402
import depth_ref as D  # noqa: E402
from varkoder_amd import _capi, cli, depth  # noqa: E402

OPEN = 2 ** 32 - 1


def test_the_two_statements_agree_on_every_case():
    calls = 0
    for c in DC.ALL_CASES + DC.FORCED_CASES:
        for every in c.everys:
            for bands in c.bandsets:
                for text, (lo, hi) in zip(c.samples, bands):
                    a = D.depth_sort(text, c.k, every, lo, hi, c.slots)
                    b = D.depth_count(text, c.k, every, lo, hi, c.slots)
                    assert (a[0], a[1], a[2], a[3]) == (b[0], b[1].tolist(), b[2], b[3]), (c.name, every, lo, hi)
                    assert sum(a[1][D.HIST_AT:]) == a[1][D.IN] and len(a[0]) <= len(text)
                    calls += 1
    assert calls >= 258


def flags(name, lo, hi, every=1, sample=0):
    c = DC.BY_NAME[name]
    return D.depth_sort(c.samples[sample], c.k, every, lo, hi, c.slots)


@pytest.mark.parametrize("k", DC.KS)
def test_what_the_cases_are_for(k):
    # n = 0 .. 4: reads of K - 1, K .. K + 3 bases, all N, empty; depths of the read's k-mers 4, 6, 3, 6
    f = lambda lo, hi: flags("n_0_to_4_k%d" % k, lo, hi)[3][:7]   # noqa: E731
    assert f(0, OPEN) == [True] * 7 and f(1, OPEN) == [False, True, True, True, True, False, False]
    assert f(0, 0) == [True, False, False, False, False, True, True]
    assert f(5, OPEN)[2] is False and f(0, 4)[2] is True     # n = 2, depths 4 and 6: the lower one decides
    assert f(4, 4) == [False, True, True, True, True, False, False]   # sorted 4 | 4 6 | 3 4 6 | 3 4 6 6: the lower median
    assert flags("n_0_to_4_k%d" % k, 0, 0)[1][D.NO_WINDOWS] == 3
    # 3 of depth 5 and 2 of depth 1: 5; 2 and 3: 1; 2 and 2: 1 (the records at 0, 5, 10)
    f = lambda lo, hi: flags("median_at_the_edges_k%d" % k, lo, hi)[3][0:15:5]   # noqa: E731
    assert f(5, OPEN) == [True, False, False] and f(6, OPEN) == [False] * 3 and f(2, OPEN) == [True, False, False]
    assert f(0, 1) == [False, True, True] and f(0, 5) == [True] * 3 and f(0, 2) == [False, True, True] and f(1, 1) == [False, True, True]
    # above the histogram: exact decisions, one bin
    _, row, _, kept = flags("above_the_histogram_k%d" % k, 256, 257)
    assert row[D.KEPT] == 256 + 257 and row[D.HIST_AT + 254] == 254 and row[D.HIST_AT + 255] == 255 + 256 + 257 + 300
    assert flags("above_the_histogram_k%d" % k, 301, OPEN - 1)[1][D.KEPT] == 0
    assert flags("above_the_histogram_k%d" % k, 300, OPEN)[1][D.KEPT] == 300
    # the seam: both long reads (records 0 and 3) have as many windows of depth 1 as of depth 3
    assert flags("tile_seam_k%d" % k, 0, 1)[3] == [True, False, False, True, False, False]
    # conflict-heavy reads and the ordinary reads behind them
    _, row, _, kept = flags("all_lanes_on_one_bin_k%d" % k, 2, OPEN)
    assert kept == [True, False, True, False, True] and row[D.HIST_AT + 255] >= 2 and row[D.HIST_AT + 1] == 2
    # every = 16: reads without a taken window
    assert flags("random_every_k%d" % k, 0, 0, every=16)[1][D.NO_WINDOWS] > 10
    # byte for byte
    c = DC.BY_NAME["byte_for_byte_k%d" % k]
    for i, t in enumerate(c.samples):
        assert flags(c.name, 0, OPEN, sample=i)[0] == t
        kept = flags(c.name, 2, OPEN, sample=i)
        assert kept[3].count(True) == 4 and kept[0] in (t[:len(kept[0])], t[len(t) - len(kept[0]):])


def test_parse_band():
    assert depth.parse_band("2:40")[1:] == (2, 40) and depth.parse_band(":4")[1:] == (None, 4)
    assert depth.parse_band("20:")[1:] == (20, None) and depth.parse_band("3x:")[1:] == (3.0, None)
    assert depth.parse_band("0.5x:2.5x")[1:] == (0.5, 2.5) and depth.parse_band(".5x:7")[1:] == (0.5, 7)
    assert depth.parse_band(" 1:1 ").text == "1:1" and depth.parse_band("5x:2") == depth.Band("5x:2", 5.0, 2)
    assert depth.parse_band("0:4294967295")[1:] == (0, OPEN)
    for bad in (":", "", "3", "1:2:3", "a:b", "-1:4", "1.5:3", "x:", "3X:", "2:1", "1e3x:", "0:4294967296", "3 x:"):
        with pytest.raises(ValueError):
            depth.parse_band(bad)


def test_resolve():
    est = {"kmer_coverage": 7.3, "reason": None}
    none = {"kmer_coverage": None, "reason": "too few repeated k-mers"}
    r = lambda text, e=est: depth.resolve(depth.parse_band(text), e)   # noqa: E731
    assert r("2:40") == (2, 40, True, None) and r(":4") == (0, 4, True, None) and r("20:") == (20, OPEN, True, None)
    # LO rounds up, HI rounds down
    assert r("3x:") == (math.ceil(3 * 7.3), OPEN, True, None) == (22, OPEN, True, None)
    assert r(":3x") == (0, 21, True, None) and r("0.5x:2x") == (4, 14, True, None)
    assert r("1x:1x", {"kmer_coverage": 5.0, "reason": None}) == (5, 5, True, None)
    assert r("2:3x") == (2, 21, True, None)
    # integers need no estimate
    assert r("2:40", none) == (2, 40, True, None)
    # no estimate: not applied, whole -- the integer end is not applied alone
    for text in ("3x:", ":2x", "2:3x", "1x:400"):
        lo, hi, applied, reason = r(text, none)
        assert (lo, hi, applied) == (0, OPEN, False) and "too few repeated k-mers" in reason
    # a band that resolves to nothing is not applied either
    lo, hi, applied, reason = r("3x:5")
    assert (lo, hi, applied) == (0, OPEN, False) and "22:5" in reason
    assert r("1000000000x:") == (OPEN, OPEN, True, None)


def test_report_and_columns():
    row = np.zeros(_capi.VK_DEPTH_NSTAT, dtype=np.uint64)
    row[:5] = (100, 60, 15000, 9000, 3)
    row[_capi.VK_DEPTH_HIST + 0], row[_capi.VK_DEPTH_HIST + 2], row[_capi.VK_DEPTH_HIST + 255] = 10, 85, 5
    band = depth.parse_band("2:")
    got = depth.report(row, band, (2, OPEN), True, None)
    assert got == {"band": "2:", "lo": 2, "hi": None, "applied": True, "reason": None, "reads_in": 100, "reads_kept": 60,
                   "bases_in": 15000, "bases_kept": 9000, "reads_without_windows": 3, "median_depth_histogram": [10, 0, 85],
                   "median_depth_255_and_more": 5}
    import json
    json.dumps(got)
    skipped = depth.report(row, depth.parse_band("3x:9"), depth.UNFILTERED, False, "why")
    assert (skipped["lo"], skipped["hi"], skipped["applied"], skipped["reason"], skipped["band"]) == (0, None, False, "why", "3x:9")
    assert depth.report(row, band, (2, 7), True, None)["hi"] == 7
    assert depth.columns(row) == {"depth_reads_in": 100, "depth_reads_removed": 40, "depth_basepairs_removed": 6000}
    assert (depth.NSTAT, depth.HIST_AT) == (D.NSTAT, D.HIST_AT) == (261, 5)


def test_refusals(tmp_path, capsys, monkeypatch):
    """exit 2, before anything runs, naming the flag; nothing is written"""
    monkeypatch.chdir(tmp_path)
    q = ["query", "-l", "m.pt", "--vocab", "v.txt", "in", "out"]
    for argv in (["image", "in", "--from-clean", "--depth-filter", "2:"],                 # without --kmer-spectrum
                 q + ["--depth-filter", ":4"],
                 ["image", "in", "--from-raw", "--kmer-spectrum", "d", "--depth-filter", ":"],
                 ["image", "in", "--from-raw", "--kmer-spectrum", "d", "--depth-filter", "4"],
                 ["image", "in", "--from-clean", "--kmer-spectrum", "d", "--depth-filter", "5:2"],
                 q + ["--kmer-spectrum", "d", "--depth-filter", "2y:"],
                 ["image", "in", "--from-bam", "--kmer-spectrum", "d", "--depth-filter", "1.5:3"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2 and "--depth-filter" in capsys.readouterr().err, argv
    assert not list(tmp_path.iterdir())
    for argv, want in ((["image", "in", "--from-raw", "--kmer-spectrum", "d", "--depth-filter", ":4"], (None, 4)),
                       (q + ["--kmer-spectrum", "d", "--depth-filter", "3x:"], (3.0, None)),
                       (["image", "in", "--from-clean", "--kmer-spectrum", "d", "--depth-filter", "5x:2"], (5.0, 2))):
        opt = cli.spectrum_options(cli.parse_args(argv))
        assert (opt.band.lo, opt.band.hi) == want
    assert cli.spectrum_options(cli.parse_args(["image", "in", "--from-clean", "--kmer-spectrum", "d"])).band is None
