"""`--from-bam` on the GPU: ImageEngine.bam_frame / bam_fastq / bam_to_fastq against tests/bam_ref.py, byte for byte:
the texts of the streams ALL, READ1, READ2 and SINGLE of every file of bam_cases.unit_cases in ONE call, the statuses, the
read counts; with VKIMG_BAM_SEG_BYTES = 256 in one engine and at its default in another, each with and without
VK_BAM_NO_GUESS.  The files lie at every residue of 4 in a buffer of sentinel bytes and the texts in slots of exactly their
size between sentinel bytes: what lies outside a file or a slot must come back untouched."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_cases as BC  # noqa: E402
import bam_ref as BR  # noqa: E402

pytestmark = pytest.mark.gpu
SEGS = ("small", "default")
SELECTS = (BR.ALL, BR.READ1, BR.READ2, BR.SINGLE)
IN_SENTINEL, OUT_SENTINEL, GAP = 0xA5, 0x5A, 37


@pytest.fixture(scope="module")
def bam_engines():
    """"small" | "default" -> an ImageEngine whose context was made with VKIMG_BAM_SEG_BYTES = 256 or unset."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(seg):
        if seg not in cache:
            old = os.environ.pop("VKIMG_BAM_SEG_BYTES", None)
            try:
                if seg == "small":
                    os.environ["VKIMG_BAM_SEG_BYTES"] = str(BC.SMALL_SEG)
                cache[seg] = ImageEngine(k=7, mapping="cgr", device=0)
            finally:
                os.environ.pop("VKIMG_BAM_SEG_BYTES", None)
                if old is not None:
                    os.environ["VKIMG_BAM_SEG_BYTES"] = old
        return cache[seg]
    yield get
    for e in cache.values():
        e.close()


@functools.lru_cache(maxsize=None)
def expected(exclude=BR.EXCLUDE_DEFAULT):
    """(cases as (name, bytes, first_record, n_ref), what the rule makes of each): computed once, shared, left unchanged."""
    cases = [(name, data) + BR.header_end(data) for name, data in BC.unit_cases()]
    return cases, [BR.convert(data, first, exclude) for _, data, first, _ in cases]


def convert(eng, cases, flags=0, exclude=BR.EXCLUDE_DEFAULT, selects=SELECTS):
    """Every stream of `selects` of every file, in one framing call and one text call.  Returns (per file {select: text},
    per file {select: reads}, status per file); asserts that no sentinel byte outside a file or a text slot changed."""
    import torch
    offs, lens, pos = [], [], 5
    for i, (_, data, _, _) in enumerate(cases):
        pos += (-pos) % 4 + i % 4   # every residue of 4
        offs.append(pos)
        lens.append(len(data))
        pos += len(data) + GAP
    host = np.full(pos + 64, IN_SENTINEL, dtype=np.uint8)
    for o, (_, data, _, _) in zip(offs, cases):
        host[o:o + len(data)] = np.frombuffer(data, dtype=np.uint8)
    dev = torch.from_numpy(host).to(eng.device)
    first = [c[2] for c in cases]
    n_ref = [c[3] for c in cases]
    sfile = [i for i in range(len(cases)) for _ in selects]
    ssel = [s for _ in cases for s in selects]
    recs, nbytes, status = eng.bam_frame(dev, offs, lens, first, n_ref, sfile, ssel, exclude=exclude, flags=flags)
    oo, at = [], 3
    for n in nbytes:
        oo.append(at)
        at += int(n) + GAP
    out = torch.full((at + 64,), OUT_SENTINEL, dtype=torch.uint8, device=eng.device)
    got, status2 = eng.bam_fastq(dev, offs, lens, first, n_ref, sfile, ssel, out, oo, nbytes, exclude=exclude, flags=flags)
    assert np.array_equal(status, status2) and np.array_equal(got, nbytes)
    assert np.array_equal(dev.cpu().numpy(), host)   # (the input, sentinels and all)
    text = out.cpu().numpy()
    mask = np.ones(len(text), dtype=bool)
    texts, counts = [], []
    for i in range(len(cases)):
        texts.append({})
        counts.append({})
        for j, s in enumerate(selects):
            k = i * len(selects) + j
            o, n = oo[k], int(nbytes[k])
            texts[i][s] = text[o:o + n].tobytes()
            counts[i][s] = int(recs[k])
            mask[o:o + n] = False
    assert (text[mask] == OUT_SENTINEL).all(), "a byte outside a stream's slot was written"
    return texts, counts, status


@pytest.mark.parametrize("no_guess", (False, True))
@pytest.mark.parametrize("seg", SEGS)
def test_texts_and_statuses_equal_the_rule(bam_engines, seg, no_guess):
    """Names of 1, 2..5 and 254 bytes; l_seq 1, 2, 63, 64, 65, 151, 2000 (records longer than several small segments,
    segments that start no record); cigars and aux data; reverse reads of odd length with every IUPAC code; absent
    qualities; a block_size word across a seam at each byte; the decoy array; files without records, with only excluded
    records, with first records at three offsets; a record cut short and bad records (no text, the status, sentinels
    intact); 300 KB of mixed reads."""
    from varkoder_amd import _capi
    eng = bam_engines(seg)
    cases, want = expected()
    texts, counts, status = convert(eng, cases, flags=_capi.VK_BAM_NO_GUESS if no_guess else 0)
    segments, rewalked = eng.last_bam_frame()
    unit = BC.SMALL_SEG if seg == "small" else 65536
    assert segments == sum(max(1, -(-len(d) // unit)) for _, d, _, _ in cases)
    for (name, _, _, _), gt, gc, gs, (ws, wt, wc) in zip(cases, texts, counts, status, want):
        assert int(gs) == ws, name
        assert gc == wc, name
        for s in SELECTS:
            assert gt[s] == wt[s], (name, s)
    by_name = dict(zip((c[0] for c in cases), status))
    assert by_name["truncated"] == BR.TRUNCATED and by_name["bad_block_size"] == BR.BAD_RECORD
    if no_guess:
        assert rewalked > 0 if segments > len(cases) else rewalked == 0
    elif seg == "small":
        assert 0 < rewalked < segments // 4   # (the decoy, records longer than a segment: most guesses are right)


@pytest.mark.parametrize("seg", SEGS)
def test_exclude_and_single_stream(bam_engines, seg):
    """--bam-exclude 0xF00; and a call whose only streams are ALL (what the default run asks for)."""
    eng = bam_engines(seg)
    cases, want = expected(0xF00)
    texts, _, status = convert(eng, cases, exclude=0xF00, selects=(BR.ALL,))
    for (name, _, _, _), gt, gs, (ws, wt, _) in zip(cases, texts, status, want):
        assert int(gs) == ws and gt[BR.ALL] == wt[BR.ALL], name
    plain = dict(zip((c[0] for c in cases), expected()[1]))
    assert plain["flags"][1][BR.ALL] != dict(zip((c[0] for c in cases), want))["flags"][1][BR.ALL]


def test_a_slot_too_small_is_left_alone(bam_engines):
    """A stream whose text does not fit its slot: VK_ENOSPC, nothing written there, the other stream written."""
    import torch
    from varkoder_amd import _capi
    eng = bam_engines("small")
    cases, want = expected()
    name, data, first, n_ref = next(c for c in cases if c[0] == "flags")
    wt = dict(zip((c[0] for c in cases), want))["flags"][1]
    dev, offs, lens = eng.upload([data])
    out = torch.full((len(wt[BR.ALL]) + len(wt[BR.READ1]) + 64,), OUT_SENTINEL, dtype=torch.uint8, device=eng.device)
    caps = [len(wt[BR.ALL]) - 1, len(wt[BR.READ1])]
    oo = [0, len(wt[BR.ALL]) + 8]
    with pytest.raises(_capi.VkError) as err:
        eng.bam_fastq(dev, offs, lens, [first], [n_ref], [0, 0], [BR.ALL, BR.READ1], out, oo, caps)
    assert err.value.status == _capi.VK_ENOSPC
    text = out.cpu().numpy()
    assert (text[:oo[1]] == OUT_SENTINEL).all()
    assert text[oo[1]:oo[1] + caps[1]].tobytes() == wt[BR.READ1]


@pytest.mark.parametrize("seg", SEGS)
def test_bam_file_through_upload_files(bam_engines, seg, tmp_path):
    """A .bam written with 300-byte BGZF members: inflated in HBM by upload_files, its header read by bam.bam_header,
    converted by bam_to_fastq."""
    from varkoder_amd import bam
    eng = bam_engines(seg)
    cases, want = expected()
    picked = [i for i, c in enumerate(cases) if c[0] in ("names_lengths", "first_2", "truncated")]
    paths = []
    for i in picked:
        p = tmp_path / (cases[i][0] + ".bam")
        p.write_bytes(BC.bgzf(cases[i][1], member=300))
        paths.append(p)
    heads = [bam.bam_header(p) for p in paths]
    assert [(h[0], h[1]) for h in heads] == [(cases[i][2], cases[i][3]) for i in picked]
    dev, offs, lens = eng.upload_files(paths)
    assert [int(n) for n in lens] == [len(cases[i][1]) for i in picked]
    out, oo, ol, status = eng.bam_to_fastq(dev, offs, lens, [h[0] for h in heads], [h[1] for h in heads], range(len(picked)),
                                           [BR.ALL] * len(picked))
    text = out.cpu().numpy()
    for j, i in enumerate(picked):
        ws, wt, _ = want[i]
        assert int(status[j]) == ws, cases[i][0]
        assert text[int(oo[j]):int(oo[j]) + int(ol[j])].tobytes() == wt[BR.ALL], cases[i][0]
