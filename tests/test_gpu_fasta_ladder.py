"""`image --from-fasta --fragments` on the GPU: vk_count_fasta_sampled_device against tests/fasta_ladder_ref.py
(histograms, taken bytes, statuses and sequence bytes equal, k = 5..9), with VKIMG_FASTA_UNIT_BYTES = 256 in one engine
and unset in another; several pairs of one sample; the error codes; the command.

The steps are the product L in {k, k + 1, 64, 150} x threshold in {0, 1, 2^31, 2^32 - 1, 2^32} x shift in {0, 1, L - 1,
2^32 - 70, 2^40 + 3} x two seeds (fasta_ladder_ref.steps), dealt over the cases of a group (fasta_ladder_ref.thinned: every
case gets steps at every L, and every combination comes up again and again across the cases), and a call takes at most
PAIRS_PER_CALL pairs, so that its histograms stay under 256 MiB at k = 9.  L = k puts a fragment seam at every offset
inside every lane, wave and unit seam of the sweeps; the large shifts exercise the 64-bit ordinal arithmetic; threshold
2^32 pins "every fragment taken, seam windows still dropped"; threshold 0 pins the full skip."""
import functools
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fasta_cases as FC  # noqa: E402
import fasta_ladder_ref as LR  # noqa: E402
import fasta_ref as FR  # noqa: E402

pytestmark = pytest.mark.gpu
KS = FC.KS
UNITS = ("small", "default")
PAIRS_PER_CALL = 192   # (192 MiB of histograms at k = 9)
POLY_A_STEPS = ((1 << 31, "L-1", 7), (LR.ALL, (1 << 40) + 3, 0x9E3779B97F4A7C15), (LR.ALL - 1, 1, 7))


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


GROUPS = {"small": (FC.small_cases, 3), "seams_small": (lambda k: FC.seam_cases(k, FC.SMALL_UNIT), 1), "batch": (FC.batch_cases, 2),
          "poly_a": (lambda k: FC.poly_a(), 0), "seams_span": (FC.span_seam_cases, 3)}


@functools.lru_cache(maxsize=None)
def expected(group, k):
    """(cases, [(status, bases)], {L: [(case index, seed, threshold, shift, codes, counts, taken)]}) of a group (codes,
    counts: sparse()): computed once, shared by the engines, left unchanged."""
    make, per_case = GROUPS[group]
    cases = make(k)
    whole = [(FR.status(d), 0 if FR.status(d) else FR.bases(d)) for _, d in cases]
    by_len = {}
    for L in (k, k + 1, 64, 150):
        if per_case:
            steps = LR.thinned(k, L, len(cases), per_case)
        else:
            steps = [[(L, seed, thr, L - 1 if shift == "L-1" else shift) for thr, shift, seed in POLY_A_STEPS]] * len(cases)
        by_len[L] = [(i, seed, thr, shift) + sparse(*LR.count(cases[i][1], k, L, seed, thr, shift))
                     for i in range(len(cases)) for _, seed, thr, shift in steps[i]]
    return cases, whole, by_len


def sparse(hist, taken):
    """(the bins of a histogram that are not zero, their counts, taken): a megabyte per step at k = 9 is not kept."""
    codes = np.flatnonzero(hist)
    return codes, hist[codes], taken


def equal(row, codes, counts):
    return np.array_equal(np.flatnonzero(row), codes) and np.array_equal(row[codes], counts)


def check_group(eng, group, k):
    cases, whole, by_len = expected(group, k)
    dev, offs, lens = eng.upload([d for _, d in cases])
    for L, pairs in by_len.items():
        for at in range(0, len(pairs), PAIRS_PER_CALL):
            part = pairs[at:at + PAIRS_PER_CALL]
            hist, status, bases, taken = eng.count_fasta_sampled(dev, offs, lens, L, [p[0] for p in part], [p[1] for p in part],
                                                                 [p[2] for p in part], [p[3] for p in part])
            hist, taken = hist.cpu().numpy().view(np.uint32), taken.cpu().numpy()
            assert status.cpu().tolist() == [w[0] for w in whole], (group, L)
            assert bases.cpu().tolist() == [w[1] for w in whole], (group, L)
            for j, (i, seed, thr, shift, codes, counts, wt) in enumerate(part):
                what = (cases[i][0], L, seed, thr, shift)
                assert int(taken[j]) == wt, what
                assert equal(hist[j], codes, counts), what


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("group", ("small", "batch", "poly_a"))
def test_kernel_equals_the_rule(fa_engines, group, k, unit):
    """small_cases (line widths, CRLF, headers, breaks, empty), the batch of 64 at every 16-byte residue with an empty
    sample and a bad start among exact neighbours, and poly-A of 1 MB (every addition on one bin)."""
    check_group(fa_engines(k, unit), group, k)


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", KS)
def test_seams(fa_engines, k, unit):
    """Header length 0..320 in steps of one against units of 256 bytes (and against lanes and waves at the default
    unit); at the default unit also the seam between two workgroups."""
    check_group(fa_engines(k, unit), "seams_small", k)
    if unit == "default":
        check_group(fa_engines(k, unit), "seams_span", k)


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("k", (5, 7, 9))
def test_several_pairs_of_one_sample(fa_engines, k, unit):
    """Pairs that name one sample several times, in any order, in one call = the same pairs in calls of their own."""
    eng = fa_engines(k, unit)
    samples = [FC.fasta([(b"a", FC.seq(61, 5000, b"ACGTN")), (b"b", FC.seq(62, 3000))], 60), FC.fasta([(b"c", FC.seq(63, 2000))], None),
               b"", FC.fasta([(b"d", FC.seq(64, 900))], 7, b"\r\n")]
    dev, offs, lens = eng.upload(samples)
    L = 64
    pairs = [(3, 5, 1 << 31, 0), (0, 5, 1 << 31, 9), (0, 6, 1 << 30, 9), (1, 5, LR.ALL, 63), (0, 5, 1 << 31, 9), (2, 1, LR.ALL, 0),
             (3, 9, 3 << 30, 17), (0, 7, LR.ALL, (1 << 40) + 3), (1, 5, 0, 0), (0, 5, 1 << 31, 10)]
    together = eng.count_fasta_sampled(dev, offs, lens, L, *zip(*pairs))
    th, tt = together[0].cpu().numpy(), together[3].cpu().numpy()
    assert together[2].cpu().tolist() == [FR.bases(s) for s in samples]
    for j, p in enumerate(pairs):
        h, _, _, t = eng.count_fasta_sampled(dev, offs, lens, L, [p[0]], [p[1]], [p[2]], [p[3]])
        assert np.array_equal(h.cpu().numpy()[0], th[j]) and int(t[0]) == int(tt[j]), p
        wh, wt = LR.count(samples[p[0]], k, L, p[1], p[2], p[3])
        assert np.array_equal(th[j].view(np.uint32), wh) and int(tt[j]) == wt, p
    assert np.array_equal(th[1], th[4]) and not np.array_equal(th[1], th[9])


def test_error_codes_launch_nothing(fa_engines):
    """frag_len = k - 1, frag_len = 2^31 and a pair_sample out of range: VK_EINVAL, and no output is touched."""
    import torch
    from varkoder_amd import _capi
    from varkoder_amd.engine import _u32, _u64
    k = 7
    eng = fa_engines(k, "default")
    dev, offs, lens = eng.upload([FC.fasta([(b"a", FC.seq(61, 5000))], 60)] * 2)
    offs, lens = np.ascontiguousarray(offs, dtype=np.uint64), np.ascontiguousarray(lens, dtype=np.uint64)
    out = [torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=eng.device) for shape in ((2, 4 ** k), (2,), (4,), (4,))]
    seeds, thr, shifts = (np.array(v, dtype=np.uint64) for v in ([1, 2], [LR.ALL, LR.ALL], [0, 0]))

    def call(frag_len, pair_sample):
        ps = np.array(pair_sample, dtype=np.uint32)
        return eng.L.vk_count_fasta_sampled_device(eng.ctx, eng._ptr(dev), _u64(offs), _u64(lens), 2, k, frag_len, 2, _u32(ps),
                                                   _u64(seeds), _u64(thr), _u64(shifts), *(eng._ptr(t) for t in out))
    for frag_len, ps in ((k - 1, [0, 1]), (1 << 31, [0, 1]), (64, [0, 2]), (64, [0xFFFFFFFF, 0])):
        assert call(frag_len, ps) == _capi.VK_EINVAL, (frag_len, ps)
    torch.cuda.synchronize()
    for t in out:
        assert bool((t == 0x5A5A5A5A).all())
    with pytest.raises(Exception):
        eng.count_fasta_sampled(dev, offs, lens, k - 1, [0], [1], [LR.ALL], [0])
    assert call(k, [1, 0]) == 0   # (the smallest fragment length is taken)
    torch.cuda.synchronize()
    assert out[1].tolist() == [0, 0] and not bool((out[0] == 0x5A5A5A5A).any())


# ---- the command ------------------------------------------------------------------------------------

def command_files(root, plain=False):
    """test_gpu_fasta.py's command_files rebuilt (three good files -- one .gz, one CRLF and unwrapped, one with an empty
    record and lower case --, a bad start, no base), and a sample below -m; plain: the .gz one as a plain file."""
    src = root / ("fasta_plain" if plain else "fasta")
    src.mkdir()
    good = {
        "mito": FC.fasta([(b"NC_000001 mitochondrion", FC.seq(901, 16569))], 70),
        "plastid.v2": FC.fasta([(b"contig1", FC.seq(902, 40000, b"ACGTacgtN")), (b"empty", b""), (b"contig2", FC.seq(903, 9000))], None, b"\r\n"),
        "scaffolds": FC.fasta([(b"s%d" % i, FC.seq(910 + i, 700 + 37 * i)) for i in range(40)], 60),
    }
    (src / "mito.fa").write_bytes(good["mito"])
    (src / "plastid.v2.fasta").write_bytes(good["plastid.v2"])
    if plain:
        (src / "scaffolds.fna").write_bytes(good["scaffolds"])
    else:
        (src / "scaffolds.fna.gz").write_bytes(gzip.compress(good["scaffolds"]))
    (src / "reads.fa").write_bytes(b"@r\nACGTACGTACGT\n+\nIIIIIIIIIIII\n")
    (src / "nobase.fa").write_bytes(b">only a header\n")
    (src / "tiny.fa").write_bytes(FC.fasta([(b"t", FC.seq(904, 5000))], 60))
    (src / "notes.txt").write_bytes(b"not a sample\n")
    return src, good


ALL_SAMPLES = ["mito", "nobase", "plastid.v2", "reads", "scaffolds", "tiny"]


@pytest.mark.parametrize("k,mapping", [(7, "cgr"), (9, "varKode")])
def test_image_fragments_command(tmp_path, k, mapping):
    import pandas as pd
    from PIL import Image
    from oracle import oracle
    from varkoder_amd import cli
    from varkoder_amd.mapping import pixel_lut, side
    from varkoder_amd.subsample import sites_ladder, threshold
    src, good = command_files(tmp_path)
    L, min_bp, out = 64, 10000, tmp_path / "images"
    common = ["image", str(src), "--from-fasta", "-k", str(k), "-p", mapping]
    cli.main(common + ["--fragments", "--fragment-length", str(L), "-m", "10K", "-M", "0", "-R", "7", "-o", str(out),
                       "-f", str(tmp_path / "stats.csv")])
    npix = side(k, mapping) ** 2
    pix = oracle.cgr_lut(k) if mapping == "cgr" else np.ascontiguousarray(pixel_lut(k, mapping), dtype=np.uint32)
    seeds = cli.draw_seeds(ALL_SAMPLES, 7)
    names, sizes = [], {}
    for s, data in good.items():
        B = FR.bases(data)
        sizes[s] = sites_ladder(B, min_bp, None)
        assert sizes[s][0] == B and len(sizes[s]) >= 2
        for level, bp in enumerate(sizes[s]):
            if level == 0:
                fq = FR.to_fastq(data)
            else:
                seed = seeds[s] + level
                kept, _ = LR.pieces(data, L, seed, threshold(bp, B), LR.shift_of(seed, L))
                fq = LR.to_fastq(kept)
            want, _, st = oracle.fastq_to_image(fq, k, pix, npix)
            assert st == 0
            names.append(f"{s}@{str(bp // 1000).rjust(8, '0')}K+{mapping}+k{k}.png")
            assert np.array_equal(np.array(Image.open(out / names[-1])).ravel(), want), names[-1]
    assert sorted(p.name for p in out.glob("*.png")) == sorted(names)
    stats = pd.read_csv(tmp_path / "stats.csv").set_index("sample")
    assert sorted(stats.index) == ALL_SAMPLES
    assert {"splitting_time", "splitting_bp_per_file", f"{k}mer_counting_time", f"k{k}_img_time", "base_frequencies_sd",
            "failed_step"} == set(stats.columns)
    for s in good:
        assert stats.loc[s, "splitting_bp_per_file"] == ",".join(str(bp) for bp in sizes[s])
        assert stats.loc[s, f"{k}mer_counting_time"] > 0 and stats.loc[s, f"k{k}_img_time"] > 0 and pd.isna(stats.loc[s, "failed_step"])
    assert stats.loc["reads", "failed_step"] == "image" and stats.loc["nobase", "failed_step"] == "image"
    assert stats.loc["tiny", "failed_step"] == "split"
    # without the flag: the files and the stats columns of today
    whole = tmp_path / "whole"
    cli.main(common + ["-o", str(whole), "-f", str(tmp_path / "whole.csv")])
    today = {s: f"{s}@{str(FR.bases(d) // 1000).rjust(8, '0')}K+{mapping}+k{k}.png" for s, d in good.items()}
    today["tiny"] = f"tiny@00000005K+{mapping}+k{k}.png"
    assert sorted(p.name for p in whole.glob("*.png")) == sorted(today.values())
    for s in good:   # (a sample's whole step is its image without the flag)
        assert (whole / today[s]).read_bytes() == (out / today[s]).read_bytes()
    assert {f"{k}mer_counting_time", f"k{k}_img_time", "base_frequencies_sd", "failed_step"} == set(pd.read_csv(tmp_path / "whole.csv").columns) - {"sample"}
    if k == 7:   # the .fna.gz input gives the plain file's images
        src2, _ = command_files(tmp_path, plain=True)
        out2 = tmp_path / "images_plain"
        cli.main(["image", str(src2), "--from-fasta", "-k", str(k), "-p", mapping, "--fragments", "--fragment-length", str(L),
                  "-m", "10K", "-M", "0", "-R", "7", "-o", str(out2), "-f", str(tmp_path / "stats2.csv")])
        assert sorted(p.name for p in out2.glob("*.png")) == sorted(names)
        for n in names:
            assert (out2 / n).read_bytes() == (out / n).read_bytes(), n
