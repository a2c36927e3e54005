"""`--from-bam --bam-read-groups` on the GPU: ImageEngine.bam_groups_frame / bam_groups_fastq / bam_groups_to_fastq against
tests/bam_groups_ref.py, byte for byte: the text of every (select, group) of every file of bam_groups_cases.unit_cases in
ONE call -- each file with its own table, truncated and bad ones among them -- the read counts and the statuses; with
VKIMG_BAM_SEG_BYTES = 256 and panels of 3 segments in one engine and both at their defaults in another.  The files lie at
every residue of 4 in a buffer of sentinel bytes and the texts in slots of exactly their size between sentinel bytes: what
lies outside a file or a slot must come back untouched."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_cases as BC  # noqa: E402
import bam_groups_cases as GC  # noqa: E402
import bam_groups_ref as GR  # noqa: E402
import bam_ref as BR  # noqa: E402

pytestmark = pytest.mark.gpu
SEGS = ("small", "default")
IN_SENTINEL, OUT_SENTINEL, GAP = 0xA5, 0x5A, 37
ENV = {"small": {"VKIMG_BAM_SEG_BYTES": str(BC.SMALL_SEG), "VKIMG_BAM_PANEL_SEGS": str(GC.SMALL_PANEL)}, "default": {}}


@pytest.fixture(scope="module")
def group_engines():
    """"small" | "default" -> an ImageEngine whose context was made with small segments and panels, or with neither set."""
    from varkoder_amd.engine import ImageEngine
    cache = {}

    def get(seg):
        if seg not in cache:
            old = {k: os.environ.pop(k, None) for k in ENV["small"]}
            try:
                os.environ.update(ENV[seg])
                cache[seg] = ImageEngine(k=7, mapping="cgr", device=0)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
        return cache[seg]
    yield get
    for e in cache.values():
        e.close()


def streams_of(ids, pairs):
    selects = (BR.SINGLE, BR.READ1, BR.READ2) if pairs else (BR.ALL,)
    return [(sel, g) for g in list(range(len(ids))) + [GR.UNGROUPED] for sel in selects]


@functools.lru_cache(maxsize=None)
def expected(exclude=BR.EXCLUDE_DEFAULT):
    """(cases as (name, bytes, first_record, n_ref, ids), (status, {(select, group): text}) of each): computed once,
    shared, left unchanged."""
    cases = [(name, data) + BR.header_end(data) + (ids,) for name, data, ids in GC.unit_cases()]
    return cases, [GR.convert(data, first, ids, exclude) for _, data, first, _, ids in cases]


def lay_out(eng, cases):
    import torch
    offs, lens, pos = [], [], 5
    for i, c in enumerate(cases):
        pos += (-pos) % 4 + i % 4   # every residue of 4
        offs.append(pos)
        lens.append(len(c[1]))
        pos += len(c[1]) + GAP
    host = np.full(pos + 64, IN_SENTINEL, dtype=np.uint8)
    for o, c in zip(offs, cases):
        host[o:o + len(c[1])] = np.frombuffer(c[1], dtype=np.uint8)
    return torch.from_numpy(host).to(eng.device), host, offs, lens


def convert(eng, cases, pairs, exclude=BR.EXCLUDE_DEFAULT, flags=0):
    """Every stream of every file in one framing call and one text call.  Returns (per file {(select, group): text}, per
    file {(select, group): reads}, status per file); asserts that no sentinel byte outside a file or a slot changed."""
    import torch
    dev, host, offs, lens = lay_out(eng, cases)
    first, n_ref, groups = [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases]
    keys = [(i,) + key for i, c in enumerate(cases) for key in streams_of(c[4], pairs)]
    sfile, ssel, sgroup = ([k[j] for k in keys] for j in range(3))
    recs, nbytes, status = eng.bam_groups_frame(dev, offs, lens, first, n_ref, groups, sfile, ssel, sgroup, exclude=exclude, flags=flags)
    oo, at = [], 3
    for n in nbytes:
        oo.append(at)
        at += int(n) + GAP
    out = torch.full((at + 64,), OUT_SENTINEL, dtype=torch.uint8, device=eng.device)
    got, status2 = eng.bam_groups_fastq(dev, offs, lens, first, n_ref, groups, sfile, ssel, sgroup, out, oo, nbytes, exclude=exclude,
                                        flags=flags)
    assert np.array_equal(status, status2) and np.array_equal(got, nbytes)
    assert np.array_equal(dev.cpu().numpy(), host)   # (the input, sentinels and all)
    text = out.cpu().numpy()
    mask = np.ones(len(text), dtype=bool)
    texts, counts = [{} for _ in cases], [{} for _ in cases]
    for k, (i, sel, g) in enumerate(keys):
        o, n = oo[k], int(nbytes[k])
        texts[i][(sel, g)] = text[o:o + n].tobytes()
        counts[i][(sel, g)] = int(recs[k])
        mask[o:o + n] = False
    assert (text[mask] == OUT_SENTINEL).all(), "a byte outside a stream's slot was written"
    return texts, counts, status


@pytest.mark.parametrize("pairs", (False, True))
@pytest.mark.parametrize("seg", SEGS)
def test_texts_counts_and_statuses_equal_the_rule(group_engines, seg, pairs):
    """1, 2, 3, 65 and 1024 groups; runs of one group longer than a wavefront, groups that alternate at every record, a
    group of the first record only, of the last only, without reads; values that are no ID; RG of other types; RG behind
    every type and subtype; each bad aux (status 3, no text) and bad aux that does not count; mates spread over groups;
    files cut short (the framing's status first), without groups, without records -- all in one call."""
    eng = group_engines(seg)
    cases, want = expected()
    texts, counts, status = convert(eng, cases, pairs)
    for (name, *_), gt, gc, gs, (ws, wt) in zip(cases, texts, counts, status, want):
        assert int(gs) == ws, name
        for key in gt:
            assert gt[key] == wt.get(key, b""), (name, key)
            assert gc[key] == wt.get(key, b"").count(b"\n") // 4, (name, key)   # (no name, base or quality is a newline)
    by_name = dict(zip((c[0] for c in cases), status))
    assert by_name["stray_1"] == GR.BAD_AUX and by_name["truncated_bad_aux"] == BR.TRUNCATED and by_name["ignored_bad"] == 0
    wgs, walked = eng.last_bam_groups()
    unit = (BC.SMALL_SEG if seg == "small" else 65536) * (GC.SMALL_PANEL if seg == "small" else 4)
    assert wgs == sum(max(1, -(-len(c[1]) // unit)) for c in cases)
    assert walked > 0


@pytest.mark.parametrize("seg", SEGS)
def test_groups_and_ungrouped_sum_to_the_plain_count(group_engines, seg):
    """Per file, the reads of all groups plus the ungrouped reads are vk_bam_frame_device's reads, class by class; also
    with --bam-exclude 0xF00 and without guesses."""
    from varkoder_amd import _capi
    eng = group_engines(seg)
    cases, want = expected(0xF00)
    good = [c for c, (ws, _) in zip(cases, want) if ws == 0]
    assert len(good) > 8
    _, counts, status = convert(eng, good, True, exclude=0xF00, flags=_capi.VK_BAM_NO_GUESS)
    assert not status.any()
    dev, _, offs, lens = lay_out(eng, good)
    selects = (BR.SINGLE, BR.READ1, BR.READ2)
    recs, _, _ = eng.bam_frame(dev, offs, lens, [c[2] for c in good], [c[3] for c in good],
                               [i for i in range(len(good)) for _ in selects], [s for _ in good for s in selects], exclude=0xF00)
    for i, c in enumerate(good):
        for j, sel in enumerate(selects):
            assert sum(n for (s, _), n in counts[i].items() if s == sel) == int(recs[3 * i + j]), (c[0], sel)
    assert sum(int(r) for r in recs) > 1000


def test_a_slot_too_small_is_left_alone(group_engines):
    """A stream whose text does not fit its slot: VK_ENOSPC, nothing written there, the other streams whole."""
    import torch
    from varkoder_amd import _capi
    eng = group_engines("small")
    cases, want = expected()
    i = next(i for i, c in enumerate(cases) if c[0] == "placement")
    name, data, first, n_ref, ids = cases[i]
    wt = want[i][1]
    keys = [(BR.ALL, ids.index(b"odd")), (BR.ALL, ids.index(b"even")), (BR.ALL, ids.index(b"run"))]
    sizes = [len(wt[k]) for k in keys]
    dev, offs, lens = eng.upload([data])
    caps = [sizes[0], sizes[1] - 1, sizes[2]]
    oo = [8, 8 + sizes[0] + 24, 8 + sizes[0] + 24 + sizes[1] + 24]
    out = torch.full((oo[2] + sizes[2] + 64,), OUT_SENTINEL, dtype=torch.uint8, device=eng.device)
    with pytest.raises(_capi.VkError) as err:
        eng.bam_groups_fastq(dev, offs, lens, [first], [n_ref], [ids], [0, 0, 0], [k[0] for k in keys], [k[1] for k in keys], out, oo, caps)
    assert err.value.status == _capi.VK_ENOSPC
    text = out.cpu().numpy()
    assert text[oo[0]:oo[0] + sizes[0]].tobytes() == wt[keys[0]]
    assert text[oo[2]:oo[2] + sizes[2]].tobytes() == wt[keys[2]]
    assert (text[:oo[0]] == OUT_SENTINEL).all() and (text[oo[0] + sizes[0]:oo[2]] == OUT_SENTINEL).all()
    assert (text[oo[2] + sizes[2]:] == OUT_SENTINEL).all()


@pytest.mark.parametrize("seg", SEGS)
def test_the_emit_grid_does_not_depend_on_the_groups(group_engines, seg):
    """The same bytes under a table of 3 groups and of 1024, with 4 streams and with 3075: the emit pass launches the same
    workgroups (one per panel) and walks the same records; the streams both calls name get the same text."""
    eng = group_engines(seg)
    cases, want = expected()
    i = next(i for i, c in enumerate(cases) if c[0] == "groups_1024")
    name, data, first, n_ref, ids = cases[i]
    dev, offs, lens = eng.upload([data])
    seen = []
    for n, pairs in ((3, False), (1024, True)):
        keys = streams_of(ids[:n], pairs)
        out, oo, ol, recs, status = eng.bam_groups_to_fastq(dev, offs, lens, [first], [n_ref], [ids[:n]], [0] * len(keys),
                                                             [k[0] for k in keys], [k[1] for k in keys])
        assert not status.any()
        text = out.cpu().numpy()
        seen.append((eng.last_bam_groups(), {k: text[int(o):int(o) + int(m)].tobytes() for k, o, m in zip(keys, oo, ol)}))
    (small, few), (large, many) = seen
    assert small == large and small[0] >= 1
    assert len(many) == 3075
    for g in (0, 1, 2):   # (group 0 has reads, 1 and 2 have none; under the short table the reads of 3.. are ungrouped)
        assert few[(BR.ALL, g)] == want[i][1].get((BR.ALL, g), b"")
        assert many[(BR.SINGLE, g)] == few[(BR.ALL, g)]   # (the case's reads are all single)
    assert few[(BR.ALL, 0)] != b"" and len(few[(BR.ALL, GR.UNGROUPED)]) > len(many[(BR.SINGLE, GR.UNGROUPED)]) > 0


def test_two_files_with_their_streams_interleaved(group_engines):
    """File 0 without groups and with one stream, its ungrouped reads; file 1 with three groups and a stream per class and
    group; file 0's stream stands in the middle of file 1's.  The smallest call in which a file's local streams are not
    the call's (ls_stream, stream_local) and a file's rows do not begin at 0 (row_first): the framing call and the text
    call against the rule."""
    import torch
    eng = group_engines("small")
    cases, want = expected()
    loose = next(c for c in cases if c[0] == "placement")
    three = next(i for i, c in enumerate(cases) if c[0] == "groups_3")
    two = [loose[:4] + ([],), cases[three]]
    rule = [GR.convert(loose[1], loose[2], [], BR.EXCLUDE_DEFAULT), want[three]]
    assert rule[0][0] == 0 and rule[1][0] == 0 and len(rule[0][1][(BR.ALL, GR.UNGROUPED)]) > 0
    keys = [(1,) + k for k in streams_of(two[1][4], True)]
    keys.insert(len(keys) // 2, (0, BR.ALL, GR.UNGROUPED))
    assert sum(len(rule[1][1].get(k[1:], b"")) > 0 for k in keys[:5]) and sum(len(rule[1][1].get(k[1:], b"")) > 0 for k in keys[7:])
    dev, host, offs, lens = lay_out(eng, two)
    a = (dev, offs, lens, [c[2] for c in two], [c[3] for c in two], [c[4] for c in two], [k[0] for k in keys], [k[1] for k in keys],
         [k[2] for k in keys])
    recs, nbytes, status = eng.bam_groups_frame(*a)
    oo = [3 + sum(int(n) + GAP for n in nbytes[:k]) for k in range(len(keys))]
    out = torch.full((oo[-1] + int(nbytes[-1]) + 64,), OUT_SENTINEL, dtype=torch.uint8, device=eng.device)
    got, status2 = eng.bam_groups_fastq(*a, out, oo, nbytes)
    assert not status.any() and not status2.any() and np.array_equal(got, nbytes)
    text = out.cpu().numpy()
    mask = np.ones(len(text), dtype=bool)
    for k, (f, sel, g) in enumerate(keys):
        wt = rule[f][1].get((sel, g), b"")
        assert text[oo[k]:oo[k] + int(got[k])].tobytes() == wt, keys[k]
        assert int(recs[k]) == wt.count(b"\n") // 4, keys[k]
        mask[oo[k]:oo[k] + int(got[k])] = False
    assert (text[mask] == OUT_SENTINEL).all(), "a byte outside a stream's slot was written"


def test_what_the_calls_refuse(group_engines):
    """VK_EINVAL before any launch: a group at or past the file's count, 1025 groups, a (file, select, group) named twice,
    VK_BAM_ALL mixed with a class select, an ID twice, an empty ID."""
    from varkoder_amd import _capi
    eng = group_engines("small")
    cases, _ = expected()
    name, data, first, n_ref, ids = next(c for c in cases if c[0] == "groups_3")
    dev, offs, lens = eng.upload([data])

    def call(groups, sel, grp):
        return eng.bam_groups_frame(dev, offs, lens, [first], [n_ref], [groups], [0] * len(sel), sel, grp)
    call(ids, [BR.ALL, BR.ALL], [0, GR.UNGROUPED])
    for groups, sel, grp in ((ids, [BR.ALL], [3]), (GC.ids_of(1025), [BR.ALL], [0]), (ids, [BR.READ1, BR.READ1], [1, 1]),
                             (ids, [BR.ALL, BR.READ1], [0, 1]), (ids[:2] + ids[:1], [BR.ALL], [0]), (ids[:2] + [b""], [BR.ALL], [0]),
                             (ids, [4], [0])):
        with pytest.raises(_capi.VkError) as err:
            call(groups, sel, grp)
        assert err.value.status == _capi.VK_EINVAL
    assert call(GC.ids_of(1024), [BR.ALL], [1023])[2][0] == 0
