"""The rule of `--from-fasta --windows` on the CPU: the two statements of tests/fasta_windows_ref.py agree on every case,
the consequences the INTEGRATION.md section states hold, and the host arithmetic (fasta.window_counts, window_names,
window_plan) and every refusal of the command line are right without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_records_ref as RR  # noqa: E402
import fasta_ref as FR  # noqa: E402
import fasta_windows_cases as WC  # noqa: E402
import fasta_windows_ref as WR  # noqa: E402

from varkoder_amd import fasta as VF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,s", WC.GEOMETRIES)
@pytest.mark.parametrize("k", (5, 9))
def test_the_two_statements_agree(k, n, s):
    for name, data in WC.all_cases(n, s) + WC.batch(n, s):
        a, b = WR.rows(data, k, n, s, WR.by_start), WR.rows(data, k, n, s, WR.by_slice)
        assert len(a) == len(b) == len(RR.joined(data)), name
        for r, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (name, r)


@pytest.mark.parametrize("k", (5, 7, 9))
def test_windows_at_step_n_sum_to_the_prefix_count(k):
    n = s = 100
    for name, data in WC.all_cases(n, s):
        for rec, rows in zip(RR.joined(data), WR.rows(data, k, n, s)):
            want = FR.count(b">x\n" + rec[:len(rows) * n + k - 1], k)[0] if len(rows) else np.zeros(4 ** k, dtype=np.uint32)
            assert np.array_equal(rows.sum(axis=0, dtype=np.uint32), want), name


@pytest.mark.parametrize("n,s", [g for g in WC.GEOMETRIES if g[0] != g[1]])
def test_a_window_is_the_sum_of_its_tiles(n, s):
    k, m = 7, n // s
    for name, data in WC.all_cases(n, s):
        for wide, tiles in zip(WR.rows(data, k, n, s), WR.rows(data, k, s, s)):
            for w in range(len(wide)):
                assert np.array_equal(wide[w], tiles[w:w + m].sum(axis=0, dtype=np.uint32)), (name, w)


def test_window_counts_at_the_edges():
    for n, s in WC.GEOMETRIES:
        assert list(VF.window_counts([0, n - 1, n, n + s - 1, n + s, n + 5 * s], n, s)) == [0, 0, 1, 1, 2, 6]
        assert [WR.nwin(b, n, s) for b in (0, n - 1, n, n + s - 1, n + s, n + 5 * s)] == [0, 0, 1, 1, 2, 6]


@pytest.mark.parametrize("m", (1, 4))
def test_window_plan_covers_every_row_once_within_the_budget(m):
    s, ncode = 25, 4 ** 5
    n = s * m
    bases = [n * 10 + 3, 5, n, n - 1, n * 3, n + s]
    row = 4 * ncode
    for budget_rows in (1, 2, 7, 9, 1000):
        win_first, ranges = VF.window_plan(bases, n, s, hist_bytes=budget_rows * row, ncode=ncode)
        counts = VF.window_counts(bases, n, s)
        at = 0
        for g, c in enumerate(counts):   # first rows: consecutive, in order; none for a record without windows
            assert win_first[g] == (at if c else VF.NO_WINDOW)
            at += int(c)
        total = at
        covered = []
        for lo, nrows, tile_rows in ranges:
            assert nrows >= 1
            covered += list(range(lo, lo + nrows))
            # the tile rows a range needs: per record with a row in it, its rows there + m - 1
            need = 0
            for g, c in enumerate(counts):
                a, b = max(lo, int(win_first[g])) if c else 0, min(lo + nrows, int(win_first[g]) + int(c)) if c else 0
                if c and a < b:
                    need += b - a + m - 1
            assert tile_rows == (need if m > 1 else 0)
            assert nrows == 1 or nrows + tile_rows <= budget_rows
        assert covered == list(range(total))
    # a small budget splits inside the first record (10 windows and more)
    _, ranges = VF.window_plan(bases, n, s, hist_bytes=(3 + (2 + m - 1 if m > 1 else 0)) * row, ncode=ncode)
    assert ranges[0][0] == 0 and ranges[0][1] < counts[0]


def test_window_plan_passes_over_duplicates_and_short_records():
    win_first, ranges = VF.window_plan([300, -1, 99, 200], 100, 100, ncode=4 ** 5)
    assert list(win_first) == [0, VF.NO_WINDOW, VF.NO_WINDOW, 3]
    assert ranges == [(0, 5, 0)]
    assert VF.window_plan([10, 20], 100, 100, ncode=4 ** 5)[1] == []


def test_window_names_parse_back():
    from varkoder_amd.convert import get_metadata_from_img_filename
    names = VF.window_names("Genus_sp__chr1.2", 10000, 2500, 3)
    assert names == ["Genus_sp__chr1.2__1-10000", "Genus_sp__chr1.2__2501-12500", "Genus_sp__chr1.2__5001-15000"]
    for nm in names:
        assert "@" not in nm and "+" not in nm
        meta = get_metadata_from_img_filename(VF.image_name(nm, 10000, 7, "cgr"))
        assert meta["sample"] == nm and meta["img_kmer_size"] == 7 and meta["img_kmer_mapping"] == "cgr" and meta["bp"] == 10000


def test_labels_fall_back_from_window_to_record_to_file():
    lab = VF.RecordLabels({"f": "file", "f__r1": "rec", "f__r1__1-100": "win"}, ["f"], windows=True)
    assert lab.get("f__r1__1-100") == "win"
    assert lab.get("f__r1__101-200") == "rec"
    assert lab.get("f__r2__1-100") == "file"
    assert lab.get("f__r2") == "file"          # (as before)
    assert lab.get("g__r2__1-100", "none") == "none"
    plain = VF.RecordLabels({"f": "file", "f__r1": "rec"}, ["f"])   # (per record, as before: no window step)
    assert plain.get("f__r1__101-200") == "file" and plain.get("f__r1") == "rec"


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "varkoder_amd.cli", *args], capture_output=True, text=True, cwd=ROOT)


IMAGE_REFUSALS = [
    ("--windows",),
    ("--from-fasta", "--windows", "--fragments"),
    ("--from-fasta", "--windows", "--per-record"),
    ("--from-fasta", "--window-length", "1000"),
    ("--from-fasta", "--window-step", "1000"),
    ("--from-fasta", "--per-record", "--window-length", "1000"),
    ("--from-fasta", "--windows", "--window-length", "99"),
    ("--from-fasta", "--windows", "--window-length", str(2 ** 31)),
    ("--from-fasta", "--windows", "--window-length", "1000", "--window-step", "300"),
    ("--from-fasta", "--windows", "--window-length", "1000", "--window-step", "2000"),
    ("--from-fasta", "--windows", "--window-length", "1000", "--window-step", "10"),     # m = 100 > 64
    ("--from-fasta", "--windows", "--window-length", "100", "--window-step", "5", "-k", "7"),   # S < k
    ("--from-fasta", "--windows", "--write-splits"),
    ("--from-fasta", "--windows", "--gpu-gzip"),
]


@pytest.mark.parametrize("extra", IMAGE_REFUSALS, ids=lambda e: " ".join(e))
def test_image_refusals_exit_2(tmp_path, extra):
    (tmp_path / "in").mkdir()
    r = _cli("image", str(tmp_path / "in"), "-o", str(tmp_path / "out"), *extra)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "--window" in r.stderr.splitlines()[-1] or "--from-fasta: not with" in r.stderr, r.stderr[-500:]   # (refused for this reason)


QUERY_REFUSALS = [
    ("--windows",),
    ("--from-fasta", "--windows", "--per-record"),
    ("--from-fasta", "--window-length", "1000"),
    ("--from-fasta", "--window-step", "1000"),
    ("--from-fasta", "--windows", "--window-length", "50"),
    ("--from-fasta", "--windows", "--window-step", "3333"),
    ("--from-fasta", "--windows", "--images"),
    ("--from-raw", "--windows"),
]


@pytest.mark.parametrize("extra", QUERY_REFUSALS, ids=lambda e: " ".join(e))
def test_query_refusals_exit_2(tmp_path, extra):
    (tmp_path / "in").mkdir()
    r = _cli("query", "-l", str(tmp_path / "m.pt"), "--vocab", str(tmp_path / "vocab.txt"), str(tmp_path / "in"), str(tmp_path / "out"), *extra)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "--window" in r.stderr.splitlines()[-1] or "--from-fasta: not with" in r.stderr, r.stderr[-500:]   # (refused for this reason)
