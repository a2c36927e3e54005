"""Step B on the MI355X at the edges that tests/clean_cases.py builds: budgets that end inside files, text behind a
file's end, lines longer than a newline chunk, more than 2^20 units, hundreds of samples and files, dirty and asymmetric
pairs, unusual framing.  The cleaned bytes, lengths, stats and status words of every sample equal clean_ref's (byte
work: no tolerance), the padding behind each sample's text is zero, vk_clean_lines_device counts what bytes.count
counts, and a second call on the same engine starts from clean tables."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adapter_ref as A  # noqa: E402
import clean_cases as K  # noqa: E402
from gpu_clean_helpers import clean, same, upload  # noqa: E402

pytestmark = pytest.mark.gpu
ON, OFF = (True, True, True), (False, False, False)


@pytest.fixture(scope="module")
def eng():
    from varkoder_amd.engine import ImageEngine
    e = ImageEngine(k=7, mapping="cgr", device=0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def batch(name, *args):
    """A builder's batch, built once and left as it is."""
    return getattr(K, name)(*args)


def with_adapters(b, F, T, flags, table):
    """expected() with adapter_ref's rule: the adapter stats as a fourth entry ([reads, bases]; a flagged sample: 0)."""
    out = []
    for (r1, r2, se, status), t in zip(K.groups(b), table):
        if status:
            out.append((b"", [0] * K.NSTAT, status, [0, 0]))
            continue
        text, st, ad = A.clean_sample_adapters(r1, r2, se, F=F, T=T, adapter=flags[0], merge=flags[1], dedup=flags[2],
                                               adapters=t)
        out.append((text, K.stats_words(st), 0, [ad["reads"], ad["bases"]]))
    return out


@pytest.mark.parametrize("F,T", K.TRIMS)
@pytest.mark.parametrize("flags", K.FLAGS)
def test_budgets(eng, flags, F, T):
    b = batch("budgets")
    got = clean(eng, b, F, T, flags)
    same(got, K.expected(b, F, T, *flags))
    names = b["names"]
    assert got[names["all_zero"]] == (b"", [0] * K.NSTAT, 0)
    assert got[names["ragged"]][2] == K.RAGGED and got[names["garbage"]][2] == 0


@pytest.mark.parametrize("flags,F,T", [(ON, 10, 10), (OFF, 0, 0)])
def test_file_ends(eng, flags, F, T):
    b = batch("file_ends")
    same(clean(eng, b, F, T, flags), K.expected(b, F, T, *flags))


@pytest.mark.parametrize("flags,F,T", [(ON, 10, 10), (OFF, 0, 0)])
def test_long_lines(eng, flags, F, T):
    b = batch("long_lines")
    same(clean(eng, b, F, T, flags), K.expected(b, F, T, *flags))


@pytest.mark.parametrize("flags,F,T", [(ON, 10, 10), (OFF, 0, 0)])
def test_many_small(eng, flags, F, T):
    b = batch("many_small")
    same(clean(eng, b, F, T, flags), K.expected(b, F, T, *flags))


@pytest.mark.parametrize("merge,dedup", [(True, True), (False, False)])
def test_many_small_with_adapters(eng, merge, dedup):
    """Every sample's own adapters: the adapter stats of a sample that shares a 256-unit workgroup with others."""
    b = batch("many_small")
    flags = (True, merge, dedup)
    want = with_adapters(b, 10, 10, flags, b["adapters"])
    assert sum(1 for w in want if w[3][0]) > 100
    same(clean(eng, b, 10, 10, flags, adapters=b["adapters"]), want)


@pytest.mark.parametrize("F,T", K.TRIMS)
@pytest.mark.parametrize("flags", K.FLAGS)
def test_dirty_pairs(eng, flags, F, T):
    b = batch("dirty_pairs", F, T)
    same(clean(eng, b, F, T, flags), K.expected(b, F, T, *flags))


@pytest.mark.parametrize("F,T", K.TRIMS)
def test_dirty_pairs_with_adapters(eng, F, T):
    b = batch("dirty_pairs", F, T)
    table = [[A.TRUSEQ1, A.TRUSEQ2, A.NEXTERA]]
    want = with_adapters(b, F, T, ON, table)
    assert want[0][3][0] > 50
    same(clean(eng, b, F, T, ON, adapters=table), want)


@pytest.mark.parametrize("flags,F,T", [(ON, 10, 10), (OFF, 0, 0)])
def test_framing(eng, flags, F, T):
    b = batch("framing")
    got = clean(eng, b, F, T, flags)
    assert [g[2] for g in got] == [0] * b["nsamples"]
    same(got, K.expected(b, F, T, *flags))


@pytest.mark.parametrize("flags", [ON, OFF])
def test_big_identity(eng, flags):
    """1,100,000 units: vk_cl_scan_top_kernel carries a total into its second round."""
    b = batch("big_identity")
    got = clean(eng, b, 0, 0, flags)
    assert got[0][0] == b["texts"][0]
    same(got, K.expected(b, 0, 0, *flags))


def test_lines_equal_a_newline_count(eng):
    tiny = K.Batch()
    rng = np.random.default_rng(1001)
    for i in range(300):
        lines = [b"x" * int(rng.integers(0, 5)) + b"\n" for _ in range(int(rng.integers(0, 9)))]
        tiny.add(b"".join(lines) + b"t" * (i % 3), K.SE, i)
    tiny["slack"] = [b"\n" * 80] * 300
    for b in (batch("file_ends"), batch("long_lines"), tiny):
        dev, offs, lens = upload(eng, b)
        assert eng.clean_lines(dev, offs, lens).tolist() == [t.count(b"\n") for t in b["texts"]]


def test_a_second_call_starts_from_clean_stats(eng):
    big, small = batch("many_small"), batch("budgets")
    want_big, want_small = K.expected(big), K.expected(small)
    assert small["nsamples"] < big["nsamples"]
    same(clean(eng, big, 10, 10, ON), want_big)
    same(clean(eng, small, 10, 10, ON), want_small)
    same(clean(eng, big, 10, 10, ON), want_big)
