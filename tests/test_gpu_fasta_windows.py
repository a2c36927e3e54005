"""`--from-fasta --windows` on the GPU: vk_count_fasta_windows_device against tests/fasta_windows_ref.py, every row
exactly equal, k = 5, 7, 8, 9, with VKIMG_FASTA_UNIT_BYTES = 64 and 128 (a span is one unit: tile seams fall in the
middle of a lane, on lane, unit and span boundaries) and step ratios m = 1, 2, 4, 64.  The cases of
tests/fasta_windows_cases.py go through one call as a batch (with a FASTQ, an empty and a header-only sample among
them, and a record without rows between selected ones); then row ranges that cut records, with canary rows around the
histogram; then every refusal.  Expected rows are computed once per (k, N, S) and left unchanged."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_windows_cases as WC  # noqa: E402
import fasta_windows_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
KS = (5, 7, 8, 9)
CANARY = 0x5A5A5A5A


@pytest.fixture(scope="module")
def fa_engines():
    """(k, unit) -> an ImageEngine whose context was made with VKIMG_FASTA_UNIT_BYTES = unit."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(k, unit):
        if (k, unit) not in cache:
            old = os.environ.get("VKIMG_FASTA_UNIT_BYTES")
            os.environ["VKIMG_FASTA_UNIT_BYTES"] = str(unit)
            try:
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
def cases_of(n, s):
    return WC.all_cases(n, s) + WC.batch(n, s)


@functools.lru_cache(maxsize=None)
def expected(k, n, s):
    """Per sample, per record: uint32 [nwin, 4^k] as sparse (window, code, count) triples."""
    out = []
    for _, d in cases_of(n, s):
        recs = []
        for rows in WR.rows(d, k, n, s):
            w, c = np.nonzero(rows)
            recs.append((rows.shape[0], w, c, rows[w, c]))
        out.append(recs)
    return out


class Batch:
    """The cases of (n, s) in HBM with their record table and a plan: every record with a window has rows but `skip`."""

    def __init__(self, eng, k, n, s):
        from varkoder_amd import fasta as VF
        self.eng, self.k, self.n, self.s, self.m = eng, k, n, s, n // s
        data = [d for _, d in cases_of(n, s)]
        self.buf = eng.upload(data)
        self.rec_first, _, self.bases, _, self.status = eng.fasta_records(*self.buf)
        want = expected(k, n, s)
        assert [int(self.rec_first[i + 1] - self.rec_first[i]) for i in range(len(data))] == [len(r) for r in want]
        counts = VF.window_counts(self.bases, n, s)
        assert list(counts) == [r[0] for recs in want for r in recs]
        with_rows = np.flatnonzero(counts)
        self.skip = int(with_rows[len(with_rows) // 2])   # a record with windows and VK_FA_NO_WINDOW between selected ones
        wanted = [-1 if g == self.skip else int(b) for g, b in enumerate(self.bases)]
        self.win_first, _ = VF.window_plan(wanted, n, s, ncode=4 ** k)
        assert self.win_first[self.skip] == VF.NO_WINDOW
        self.total = int(sum(c for g, c in enumerate(counts) if g != self.skip))
        # the expected rows, dense, on the device
        import torch
        rows, codes, vals = [], [], []
        for g, (nw, w, c, v) in enumerate(r for recs in want for r in recs):
            if nw and g != self.skip:
                rows.append(w + int(self.win_first[g]))
                codes.append(c)
                vals.append(v)
        exp = np.zeros((self.total, 4 ** k), dtype=np.uint32)
        exp[np.concatenate(rows), np.concatenate(codes)] = np.concatenate(vals)
        self.exp = torch.from_numpy(exp.view(np.int32)).to(eng.device)
        self.counts = counts

    def tile_rows(self, lo, nrows):
        if self.m == 1:
            return 0
        need = 0
        for g, c in enumerate(self.counts):
            if c and g != self.skip:
                a, b = max(lo, int(self.win_first[g])), min(lo + nrows, int(self.win_first[g]) + int(c))
                if a < b:
                    need += b - a + self.m - 1
        return max(need, 1)   # (a range without a window still states a workspace: 0 is refused)

    def count(self, lo, nrows, hist=None, tile_rows=None):
        return self.eng.count_fasta_windows(*self.buf, self.rec_first, self.bases, self.win_first, self.n, self.s, lo, nrows,
                                            self.tile_rows(lo, nrows) if tile_rows is None else tile_rows, hist=hist)


def assert_equal_rows(got, want, what):
    import torch
    if not torch.equal(got, want):
        bad = (got != want).any(dim=1).nonzero().flatten().tolist()
        raise AssertionError(f"{what}: rows differ: {bad[:10]} ({len(bad)} of {got.shape[0]})")


@pytest.mark.parametrize("n,s", WC.GEOMETRIES)
@pytest.mark.parametrize("unit", WC.UNITS)
@pytest.mark.parametrize("k", KS)
def test_every_window_of_a_batch_equals_the_rule(fa_engines, k, unit, n, s):
    """One call over all rows and two spare ones: every window's row equal, the spare rows zero."""
    import torch
    b = Batch(fa_engines(k, unit), k, n, s)
    hist = b.count(0, b.total + 2)
    torch.cuda.synchronize()
    assert_equal_rows(hist[:b.total], b.exp, "all rows")
    assert not bool(hist[b.total:].any())


@pytest.mark.parametrize("n,s", ((100, 100), (96, 24), (576, 9)))
@pytest.mark.parametrize("k,unit", ((5, 64), (7, 128), (9, 64)))
def test_row_ranges_cut_records_and_touch_nothing_else(fa_engines, k, unit, n, s):
    """The rows of [lo, lo + n) equal the slice of the one-call result, for ranges that begin and end inside records, lie
    within one record, cover one row, or reach past the last row; canary rows before and behind stay as they were."""
    import torch
    b = Batch(fa_engines(k, unit), k, n, s)
    t = b.total
    first_long = int(b.win_first[0])   # (record 0 has several windows: a range inside it)
    for lo, nrows in ((0, 1), (1, 2), (first_long + 1, 1), (2, t // 3), (t // 3 + 1, t // 2), (t - 3, 3), (t - 2, 5), (t, 4)):
        buf = torch.full((nrows + 2, 4 ** k), CANARY, dtype=torch.int32, device=b.eng.device)
        b.count(lo, nrows, hist=buf[1:nrows + 1])
        torch.cuda.synchronize()
        assert bool((buf[0] == CANARY).all()) and bool((buf[-1] == CANARY).all()), (lo, nrows)
        inside = max(0, min(nrows, t - lo))
        assert_equal_rows(buf[1:1 + inside], b.exp[lo:lo + inside], f"range {lo}+{nrows}")
        assert not bool(buf[1 + inside:nrows + 1].any()), (lo, nrows)


def test_a_tile_workspace_too_small_drops_rows_and_nothing_else(fa_engines):
    """tile_rows below what the range needs: the windows whose tiles fit are right, the others come back zero."""
    import torch
    b = Batch(fa_engines(7, 64), 7, 96, 24)
    hist = b.count(0, b.total, tile_rows=b.m + 2)   # the first three windows of the first record
    torch.cuda.synchronize()
    assert_equal_rows(hist[:3], b.exp[:3], "the windows that fit")
    assert not bool(hist[3:].any())


def test_wrong_tables_from_the_caller_stay_in_bounds(fa_engines):
    """win_first past the range, rows that overlap, bases that are not the records': wrong answers are allowed, writes
    outside the histogram are not (canary rows)."""
    import torch
    b = Batch(fa_engines(9, 64), 9, 100, 100)
    for wf, bases in ((np.full_like(b.win_first, 3), b.bases), (b.win_first + np.uint64(2 ** 40), b.bases),
                      (b.win_first, b.bases * np.uint64(3) + np.uint64(1000)), (b.win_first, np.full_like(b.bases, 2 ** 63))):
        buf = torch.full((8 + 2, 4 ** 9), CANARY, dtype=torch.int32, device=b.eng.device)
        b.eng.count_fasta_windows(*b.buf, b.rec_first, bases, wf, 100, 100, 2, 8, 0, hist=buf[1:9])
        torch.cuda.synchronize()
        assert bool((buf[0] == CANARY).all()) and bool((buf[-1] == CANARY).all())


def test_refusals(fa_engines):
    """VK_EINVAL before anything is launched."""
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import _u64
    eng = fa_engines(7, 64)
    b = Batch(eng, 7, 100, 100)
    dev, offs, lens = b.buf
    offs, lens = eng._desc(offs, lens)
    d_bases = torch.from_numpy(np.ascontiguousarray(b.bases).view(np.int64)).to(eng.device)
    d_first = torch.from_numpy(b.win_first.view(np.int64)).to(eng.device)
    hist = torch.full((4, 4 ** 7), CANARY, dtype=torch.int32, device=eng.device)
    P = eng._ptr
    good = dict(ctx=eng.ctx, text=P(dev), offs=_u64(offs), lens=_u64(lens), n=len(offs), k=7, rec_first=_u64(b.rec_first),
                bases=P(d_bases), first=P(d_first), N=100, S=100, lo=0, nrows=4, tiles=0, hist=P(hist))

    def call(**change):
        a = dict(good, **change)
        return eng.L.vk_count_fasta_windows_device(a["ctx"], a["text"], a["offs"], a["lens"], a["n"], a["k"], a["rec_first"], a["bases"],
                                                   a["first"], a["N"], a["S"], a["lo"], a["nrows"], a["tiles"], a["hist"])
    bad_first = b.rec_first.copy()
    bad_first[0] = 1
    decreasing = b.rec_first.copy()
    decreasing[1] = decreasing[2] + 1
    refused = [dict(ctx=None), dict(text=None), dict(offs=None), dict(lens=None), dict(rec_first=None), dict(bases=None),
               dict(first=None), dict(hist=None), dict(k=4), dict(k=10), dict(S=6, N=96), dict(N=100, S=30), dict(N=650, S=10),
               dict(N=2 ** 31, S=2 ** 31), dict(N=2 ** 31, S=2 ** 30), dict(nrows=0), dict(N=96, S=24, tiles=0),
               dict(rec_first=_u64(bad_first)), dict(rec_first=_u64(decreasing))]
    for change in refused:
        assert call(**change) == _capi.VK_EINVAL, change
    torch.cuda.synchronize()
    assert bool((hist == CANARY).all())   # nothing was launched, not even the zeroing
    assert call() == _capi.VK_OK
    assert call(N=640, S=10, tiles=64) == _capi.VK_OK   # m = 64 is the most
    torch.cuda.synchronize()
