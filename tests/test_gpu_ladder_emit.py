"""Step C's files on the GPU (vk_ladder_emit_device, ImageEngine.ladder_emit, subsample.ladder_files) against
tests/ladder_emit_ref.py byte for byte, and against the counts of the direct run."""
import random

import numpy as np
import pytest

import ladder_emit_ref as R
from varkoder_amd import _capi

pytestmark = pytest.mark.gpu

ALL = 1 << 32


def emit(eng, samples, steps, **kw):
    """steps = [(sample index, seed, threshold, whole)] -> (each step's text, status per sample)."""
    dev, offs, lens = eng.upload(samples)
    out, ooffs, olens, status = eng.ladder_emit(dev, offs, lens, [s[0] for s in steps], [s[1] for s in steps],
                                                [s[2] for s in steps], [s[3] for s in steps], **kw)
    host = out.cpu().numpy()
    assert all(int(o) % 16 == 0 for o in ooffs)
    for o, n in zip(ooffs, olens):   # zeros up to the 16-byte rounded end
        assert not host[int(o) + int(n):(int(o) + int(n) + 15) // 16 * 16].any()
    return [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(ooffs, olens)], status


def want(samples, steps):
    return [R.emit_ref(samples[i], seed, thr, whole=bool(w)) for i, seed, thr, w in steps]


def reads_fastq(rng, lens, tag="r"):
    parts = []
    for i, n in enumerate(lens):
        seq = "".join(rng.choice("ACGT") for _ in range(n))
        parts.append(f"@{tag}{i} len={n}\n{seq}\n+\n{'F' * n}\n")
    return "".join(parts).encode()


def test_the_rule_on_every_shared_input(engines):
    """every input of the CPU test, k = 5..9, every seed and threshold, and a whole step: one call"""
    eng = engines(7)
    samples, steps = [], []
    for k in (5, 6, 7, 8, 9):
        for text in R.case_inputs(k).values():
            i = len(samples)
            samples.append(text)
            steps += [(i, seed, thr, 0) for seed in R.SEEDS for thr in R.THRESHOLDS] + [(i, 3, 0, 1)]
    got, status = emit(eng, samples, steps)
    assert not status.any()
    exp = want(samples, steps)
    for j, st in enumerate(steps):
        assert got[j] == exp[j], st
    assert any(g == b"" for g in got) and any(b"_3\n" in g for g in got)   # (a step that takes nothing; cut reads)


def test_a_sample_alone_and_among_300_others(engines):
    eng = engines(7)
    rng = random.Random(5)
    main = reads_fastq(rng, [rng.choice((40, 150, 150, 501, 1300)) for _ in range(400)])
    mine = [(0, 11, ALL // 2, 0), (0, 12, ALL // 20, 0), (0, 0, 0, 1)]
    alone, _ = emit(eng, [main], mine)
    assert alone == want([main], mine) and all(alone)
    tiny = [reads_fastq(rng, [rng.randrange(0, 80) for _ in range(rng.randrange(1, 6))], tag="t%d." % i) for i in range(300)]
    samples = tiny[:137] + [main] + tiny[137:]
    steps = []
    for i in range(len(samples)):
        if i == 137:
            steps += [(137,) + st[1:] for st in mine]
        else:
            steps += [(i, 5 + j, ALL // (j + 1), int(j == 2)) for j in range(i % 4)]   # 0 .. 3 steps
    got, status = emit(eng, samples, steps)
    assert not status.any()
    assert got == want(samples, steps)
    at = steps.index((137,) + mine[0][1:])
    assert got[at:at + 3] == alone


def test_every_residue_of_16(engines):
    """A sample starts at a multiple of 16 bytes (the ABI's rule for every count call); its records, its end and its
    files' records lie at every residue."""
    eng = engines(7)
    rng = random.Random(16)
    base = reads_fastq(rng, [150, 33, 501, 64, 1001])
    samples = [b"@" + b"p" * r + base[1:] for r in range(16)]   # (a longer first header moves everything behind it)
    assert {len(s) % 16 for s in samples} == set(range(16))
    steps = [(i, 1, ALL, 0) for i in range(16)] + [(i, 2, ALL // 2, 0) for i in range(16)] + [(i, 0, 0, 1) for i in range(16)]
    got, _ = emit(eng, samples, steps)
    assert got == want(samples, steps)
    # the sample's own start is the ABI's multiple of 16, as for every count call: anything else is refused unread
    dev, offs, lens = eng.upload(samples[:2])
    assert offs[1] % 16 == 0
    for r in range(1, 16):
        with pytest.raises(_capi.VkError) as err:
            eng.ladder_emit(dev, [0, int(offs[1]) + r], [int(lens[0]), int(lens[1]) - r], [1], [1], [ALL], [0], records=[5, 5])
        assert err.value.status == _capi.VK_EINVAL


def test_records_across_chunks_and_slices(engines):
    """4,097 reads of 150 bases: records straddle the 16 KiB chunks of the newline passes, the scan blocks of 4,096
    items and the write kernel's workgroups; ladder_files in several slices gives the same files"""
    from varkoder_amd.subsample import ladder_files, ladder_plan
    eng = engines(7)
    rng = random.Random(4097)
    text = reads_fastq(rng, [150] * 4097)
    steps = [(0, 1, ALL // 2, 0), (0, 2, ALL // 50, 0), (0, 0, ALL, 0), (0, 0, 0, 1)]
    got, _ = emit(eng, [text], steps)
    assert got == want([text], steps)
    small = reads_fastq(rng, [150] * 100, tag="s")
    dev, offs, lens = eng.upload([text, small])
    nsites, status = eng.read_index(dev, offs, lens)
    assert nsites.tolist() == [4097 * 150, 100 * 150]
    files = {}
    for slice_bytes in (1 << 30, 1000):
        found = {}
        for out, part in ladder_files(eng, dev, offs, lens, nsites, status, seed=9, min_bp=2000, max_bp=300000,
                                      slice_bytes=slice_bytes):
            host = out.cpu().numpy()
            for i, bp, o, n in part:
                found[(i, bp)] = host[o:o + n].tobytes()
        files[slice_bytes] = found
    assert files[1000] == files[1 << 30] and len(files[1000]) >= 8
    _, plans = ladder_plan(nsites, status, 2000, 300000)
    from varkoder_amd.subsample import threshold
    for (i, bp), body in files[1000].items():
        level = plans[i].index(bp)
        whole = level == 0 and bp >= nsites[i]
        assert body == R.emit_ref([text, small][i], 9 + level, threshold(bp, nsites[i]), whole=whole), (i, bp)


def test_bad_framing_beside_good_samples(engines):
    eng = engines(7)
    rng = random.Random(3)
    good = reads_fastq(rng, [150, 600, 20])
    bad = [good[1:], good.replace(b"\n+\n", b"\n-\n", 1), good + b"@x\nAC\n", b"@r\nAC\n+\n"]
    samples = [good] + bad + [good[:good.index(b"@r1")]]
    steps = [(i, 4, ALL, w) for i in range(len(samples)) for w in (0, 1)]
    got, status = emit(eng, samples, steps)
    assert status.tolist() == [R.framing_status(s) for s in samples]
    assert status[0] == 0 and status[-1] == 0 and all(status[1:-1])
    assert got == want(samples, steps)
    assert got[0] and got[-1] and not any(got[2:-2])
    # the records the caller states are checked against the text
    dev, offs, lens = eng.upload([good])
    _, _, _, st = eng.ladder_emit(dev, offs, lens, [0], [0], [ALL], [1], records=[2])
    assert st.tolist() == [_capi.VK_EM_BAD_RECORDS]


def test_a_buffer_one_byte_short(engines):
    import torch
    eng = engines(7)
    rng = random.Random(8)
    text = reads_fastq(rng, [150, 700, 90, 1200])
    dev, offs, lens = eng.upload([text])
    steps = ([0, 0], [1, 2], [ALL, ALL], [0, 1])
    exp = want([text], [(0, 1, ALL, 0), (0, 2, ALL, 1)])
    need = sum((len(e) + 15) // 16 * 16 for e in exp)
    buf = torch.full((need + 64,), 0xAB, dtype=torch.uint8, device=eng.device)
    with pytest.raises(_capi.VkError) as err:
        eng.ladder_emit(dev, offs, lens, *steps, capacity=need - 1, out=buf)
    assert err.value.status == _capi.VK_ENOSPC
    assert bool((buf == 0xAB).all())
    out, ooffs, olens, _ = eng.ladder_emit(dev, offs, lens, *steps, capacity=need, out=buf)
    host = out.cpu().numpy()
    assert [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(ooffs, olens)] == exp
    assert (host[need:] == 0xAB).all()


@pytest.mark.parametrize("k", [5, 6, 7, 8, 9])
def test_the_files_count_to_the_direct_runs_histograms(engines, k):
    """the invariant, on the device: engine.count of every emitted file = the tensor ladder_counts returned for the
    step (dense route for k <= 7, quad route for k = 8, 9; walked and streamed subsamples), sites_taken = its bases
    -- on the CRLF sample exactly one more per read taken, the '\\r' that the sites count and the files drop;
    ladder_counts with parts = 1 gives the same"""
    import torch
    from varkoder_amd.subsample import ladder_counts, ladder_files, threshold
    eng = engines(k)
    rng = random.Random(60 + k)
    a = reads_fastq(rng, [rng.choice((150, 150, 150, 90, 620, 1250)) for _ in range(500)], tag="a")
    b = reads_fastq(rng, [rng.choice((150, 499, 500, 501, 1000 + k)) for _ in range(60)], tag="b")
    c = reads_fastq(rng, [rng.choice((150, 499, 500, 501, 1000 + k)) for _ in range(60)], tag="c").replace(b"\n", b"\r\n")
    anchors = [r[0] for r in R.records(c)]
    dev, offs, lens = eng.upload([a, b, c])
    for max_bp in (None, 30000):
        recs = ladder_counts(eng, dev, offs, lens, seed=21, min_bp=2000, max_bp=max_bp)
        one = ladder_counts(eng, dev, offs, lens, seed=21, min_bp=2000, max_bp=max_bp, parts=1)
        assert all(r["error"] is None and len(r["steps"]) >= 4 for r in recs)
        nsites, status = [r["nsites"] for r in recs], [r["status"] for r in recs]
        seen = 0
        for out, part in ladder_files(eng, dev, offs, lens, nsites, status, seed=21, min_bp=2000, max_bp=max_bp):
            h, st = eng.count(out, [o for _, _, o, _ in part], [n for _, _, _, n in part])
            assert not st.cpu().numpy().any()
            host = out.cpu().numpy()
            for row, (i, bp, o, n) in enumerate(part):
                level = [s[0] for s in recs[i]["steps"]].index(bp)
                _, hist, taken = recs[i]["steps"][level]
                assert torch.equal(h[row], hist), (max_bp, i, bp)
                assert torch.equal(one[i]["steps"][level][1], hist), (max_bp, i, bp)
                dropped = 0
                if i == 2:
                    thr = threshold(bp, nsites[i])
                    dropped = sum(1 for at in anchors if (level == 0 and bp >= nsites[i]) or R.sample_hash(21 + level, at) < thr)
                    assert dropped > 0 or level > 0   # (a first step takes most reads; a small one may take none)
                assert R.emitted_bases(host[o:o + n].tobytes()) == taken - dropped, (max_bp, i, bp)
                seen += 1
        assert seen == sum(len(r["steps"]) for r in recs)
