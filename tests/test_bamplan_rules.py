"""The host rules of the BAM calls (csrc/vk_bamplan.h) on a CPU, through tests/emul/bamplan_emul.cpp: what the argument
rules refuse and the neighbour they accept, the 2^31 limits, the group table under the product's own probe, the map and
the stream tables against the rule stated here, the workspace size against what the calls stated before the rules moved
(tests/golden/bam_groups_ws.json), the result rules -- and the same cases through the sanitizer build."""
import json
import os

import pytest

import bamplan_emul_lib as EM
from bamplan_emul_lib import ALL, NO_GUESS, NO_STREAM, READ1, READ2, SINGLE, UNGROUPED

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_GROUPS, MAX_ID = 1024, 255
BAD_RECORD, TRUNCATED, BAD_AUX = 1, 2, 3


def names(n):
    return [b"rg%d" % g for g in range(n)]


# ---- refusals, each beside a neighbour that is accepted -----------------------------------------------------------------
G = [[b"a", b"b"]]          # one file, two groups
G2 = [[b"a", b"b"], [b"a"]]   # two files
ARGS = {
    # name: (case, bam_args_ok, bg_args_ok)
    "a plain call": (EM.args_case([100], [(0, ALL)]), True, False),
    "a grouped call": (EM.args_case([100], [(0, ALL, 0)], G), True, True),
    "no files and no streams": (EM.args_case([], [], []), True, True),
    "the last group of the file": (EM.args_case([100], [(0, READ1, 1)], G), True, True),
    "a group index at the file's count": (EM.args_case([100], [(0, READ1, 2)], G), True, False),
    "a group index past the file's count": (EM.args_case([100], [(0, READ1, 3)], G), True, False),
    "a group index another file has": (EM.args_case([100, 100], [(1, READ1, 1)], G2), True, False),
    "the ungrouped reads": (EM.args_case([100], [(0, READ1, UNGROUPED)], G), True, True),
    "1024 groups": (EM.args_case([100], [(0, ALL, 1023)], [names(MAX_GROUPS)]), True, True),
    "1025 groups": (EM.args_case([100], [(0, ALL, 1023)], [names(MAX_GROUPS + 1)]), True, False),
    "an empty ID": (EM.args_case([100], [], [[b"a", b"", b"c"]]), True, False),
    "an ID of 255 bytes": (EM.args_case([100], [], [[b"a", b"x" * MAX_ID]]), True, True),
    "an ID of 256 bytes": (EM.args_case([100], [], [[b"a", b"x" * (MAX_ID + 1)]]), True, False),
    "the same ID twice in one file": (EM.args_case([100], [], [[b"a", b"b", b"a"]]), True, False),
    "the same ID in two files": (EM.args_case([100, 100], [], G2), True, True),
    "an ID that is a prefix of another": (EM.args_case([100], [], [[b"ab", b"a"]]), True, True),
    "a (file, group, select) named twice": (EM.args_case([100], [(0, READ1, 0), (0, READ2, 0), (0, READ1, 0)], G), True, False),
    "a (file, group) with two selects": (EM.args_case([100], [(0, READ1, 0), (0, READ2, 0), (0, READ1, 1)], G), True, True),
    "ALL and a class on one file": (EM.args_case([100], [(0, ALL, 0), (0, READ1, 1)], G), True, False),
    "ALL and a class on two files": (EM.args_case([100, 100], [(0, ALL, 0), (1, READ1, 0)], G2), True, True),
    "a stream of the last file": (EM.args_case([100, 100], [(1, ALL)]), True, False),
    "a stream of a file past the last": (EM.args_case([100, 100], [(2, ALL)]), False, False),
    "a grouped stream of a file past the last": (EM.args_case([100, 100], [(2, ALL, 0)], G2), False, False),
    "the select SINGLE": (EM.args_case([100], [(0, SINGLE)]), True, False),
    "a select above SINGLE": (EM.args_case([100], [(0, SINGLE + 1)]), False, False),
    "the flag NO_GUESS": (EM.args_case([100], [(0, ALL, 0)], G, flags=NO_GUESS), True, True),
    "an unknown flag bit": (EM.args_case([100], [(0, ALL, 0)], G, flags=NO_GUESS | 2), False, False),
    "group_first that begins at 0": (EM.args_case([100, 100], [], G2, group_first=[0, 2, 3]), True, True),
    "group_first that begins at 1": (EM.args_case([100, 100], [], [[b"a", b"b"], [b"a", b"c"]], group_first=[1, 2, 4]), True, False),
    "a file without groups between two with": (EM.args_case([1, 1, 1], [], [[b"a"], [], [b"a"]], group_first=[0, 1, 1, 2]), True, True),
    "group_first that decreases": (EM.args_case([1, 1, 1], [], [[b"a", b"b"], [], []], group_first=[0, 2, 1, 2]), True, False),
    "id_first that begins at 1": (EM.args_case([100], [], [[b"ab", b"c"]], id_first=[1, 2, 3]), True, False),
}


@pytest.mark.parametrize("name", list(ARGS))
def test_what_the_rules_refuse(name):
    case, bam_ok, bg_ok = ARGS[name]
    assert EM.run(case) == {"bam_args_ok": bam_ok, "bg_args_ok": bg_ok}


# ---- the framing's plan and its limits: lengths only, no memory of that size is touched -----------------------------------
LIMIT = 1 << 31


def plan_want(seg, lengths, stream_file, slots=None, grouped=False):
    """The plan as the rule states it: a file has ceil(length / seg) segments and at least one; a stream has its file's."""
    segs = [max(1, -(-n // seg)) for n in lengths]
    sf = [] if grouped else list(stream_file)
    seg_first = [sum(segs[:i]) for i in range(len(segs) + 1)]
    sseg_first = [sum(segs[f] for f in sf[:i]) for i in range(len(sf) + 1)]
    slots = list(slots) if slots and not grouped else [(0, 0)] * len(sf)   # zero when the call only frames
    return {"ok": int(seg_first[-1] < LIMIT and sseg_first[-1] < LIMIT), "seg": seg, "nstreams": len(sf), "segs": seg_first[-1],
            "stream_segs": sseg_first[-1], "seg_first": seg_first, "sseg_first": sseg_first,
            "out_offs": [s[0] for s in slots], "out_caps": [s[1] for s in slots]}


def plan_pair(seg_bytes, lengths, streams, groups=None, slots=None):
    seg = seg_bytes or 65536
    return (EM.plan_case(seg_bytes, lengths, streams, groups, slots=slots),
            plan_want(seg, lengths, [s[0] for s in streams], slots, groups is not None))


PLANS = {
    "the default segment": plan_pair(0, [0, 1, 65536, 65537], [(3, ALL), (0, READ1), (3, READ2)]),
    "a zero-length file counts as one segment": plan_pair(64, [0], [(0, ALL)]),
    "odd lengths, interleaved streams": plan_pair(64, [63, 64, 65, 0, 1000], [(4, ALL), (0, READ1), (4, READ1), (2, SINGLE)]),
    "a text call's slots": plan_pair(256, [300, 10], [(1, ALL), (0, READ1)], slots=[(16, 5), (32, 700)]),
    "a grouped call frames without streams": plan_pair(256, [300, 10], [(1, ALL, 0), (0, READ1, UNGROUPED)], [[], [b"a"]]),
    "one segment short of 2^31 segments": plan_pair(64, [(LIMIT - 1) * 64], []),
    "2^31 segments": plan_pair(64, [LIMIT * 64], []),
    "2^31 segments in two files": plan_pair(64, [(LIMIT - 1) * 64, 0], []),
    "2^31 - 1 segments, a zero-length file among them": plan_pair(64, [(LIMIT - 2) * 64, 0], []),
    "2^31 - 1 stream segments": plan_pair(64, [((1 << 30) - 1) * 64, 64], [(0, READ1), (0, READ2), (1, ALL)]),
    "2^31 stream segments": plan_pair(64, [(1 << 30) * 64, 64], [(0, READ1), (0, READ2)]),
    "2^31 stream segments, a grouped call": plan_pair(64, [(1 << 30) * 64], [(0, READ1, 0), (0, READ2, 0)], [[b"a"]]),
}


def test_the_limit_cases_lie_where_they_should():
    want = {name: w for name, (_, w) in PLANS.items()}
    assert want["one segment short of 2^31 segments"]["segs"] == LIMIT - 1 and want["one segment short of 2^31 segments"]["ok"] == 1
    assert want["2^31 segments"]["segs"] == LIMIT and want["2^31 segments"]["ok"] == 0
    assert want["2^31 segments in two files"]["segs"] == LIMIT and want["2^31 segments in two files"]["ok"] == 0
    assert want["2^31 - 1 segments, a zero-length file among them"]["ok"] == 1
    assert want["2^31 - 1 stream segments"]["stream_segs"] == LIMIT - 1 and want["2^31 - 1 stream segments"]["ok"] == 1
    assert want["2^31 stream segments"]["stream_segs"] == LIMIT and want["2^31 stream segments"]["segs"] < LIMIT
    assert want["2^31 stream segments"]["ok"] == 0
    assert want["2^31 stream segments, a grouped call"]["ok"] == 1   # (its streams are the count pass's: rows, not segments)


@pytest.mark.parametrize("name", list(PLANS))
def test_the_framing_plan(name):
    case, want = PLANS[name]
    assert EM.run(case) == want


# ---- the group table, under the product's probe --------------------------------------------------------------------------
def fnv(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


def table_slots(n):
    s = 2
    while s < 2 * n:
        s <<= 1
    return s


def colliding(n):
    """n IDs of which every other one hashes into the first sixteenth of the table's slots (at least four slots)."""
    mask, ids, i = table_slots(n) - 1, [], 0
    while len(ids) < n:
        b = b"c%d" % i
        if fnv(b) & mask < max(4, (mask + 1) // 16) or len(ids) % 2:
            ids.append(b)
        i += 1
    return ids


TABLE_COUNTS = (0, 1, 2, 3, 63, 64, 65, 1023, 1024)


def table_case(n, ids):
    absent = [b"absent", b"", b"rg", b"rg%d" % n, b"c"]
    prefixes = [i[:-1] for i in ids[:8] if i[:-1] not in ids] + [i + b"0" for i in ids[:8] if i + b"0" not in ids]
    queries = [(1, i) for i in ids] + [(1, q) for q in absent + prefixes if q not in ids]
    # file 1 of three holds the table: its slice of the tables begins behind file 0's
    return EM.describe_case(256, 3, [10, 10, 10], [], [[b"x", b"y", b"z"], ids, [b"x"]], queries), len(ids)


TABLES = {f"{n} groups": table_case(n, names(n)) for n in TABLE_COUNTS}
TABLES.update({f"{n} groups that collide": table_case(n, colliding(n)) for n in TABLE_COUNTS if n > 1})


def check_table(got, nids):
    assert got["found"][:nids] == list(range(nids))
    assert len(got["found"]) > nids and set(got["found"][nids:]) == {UNGROUPED}
    assert len(got["slots"]) == table_slots(3) + table_slots(nids) + table_slots(1)
    assert got["slot_first"] == [0, table_slots(3), table_slots(3) + table_slots(nids)]
    mine = got["slots"][table_slots(3):table_slots(3) + table_slots(nids)]
    assert sorted(x for x in mine if x) == list(range(1, nids + 1))


@pytest.mark.parametrize("name", list(TABLES))
def test_every_id_is_found_at_its_own_index(name):
    case, nids = TABLES[name]
    check_table(EM.run(case), nids)


def test_the_colliding_ids_collide():
    ids = colliding(64)
    firsts = [fnv(i) & (table_slots(64) - 1) for i in ids]
    assert len(set(firsts)) <= 32 + 8   # half of them share eight slots: the probe has to step


# ---- the map and the stream tables -----------------------------------------------------------------------------------
def tables_want(seg, panel, lengths, streams, groups):
    """The rule: a file's streams are numbered in the call's order (local streams); map[(cls - 1) * (ng + 1) + slot] is the
    local stream that takes the reads of class cls of the group `slot` (ng: the ungrouped reads); a file's rows are its
    panels times its local streams."""
    nf = len(lengths)
    local, per_file = [], [[] for _ in range(nf)]
    for s, (f, _, _) in enumerate(streams):
        local.append(len(per_file[f]))
        per_file[f].append(s)
    maps = []
    for f in range(nf):
        ng = len(groups[f])
        m = [NO_STREAM] * (3 * (ng + 1))
        for s in per_file[f]:
            _, select, group = streams[s]
            for cls in (1, 2, 3):
                if select in (ALL, cls):
                    m[(cls - 1) * (ng + 1) + (ng if group == UNGROUPED else group)] = local[s]
        maps.append(m)
    npan = [-(-max(1, -(-n // seg)) // panel) for n in lengths]
    return {"map": [x for m in maps for x in m], "map_first": [sum(len(m) for m in maps[:f]) for f in range(nf)],
            "ls_first": [sum(len(p) for p in per_file[:f]) for f in range(nf + 1)], "ls_stream": [s for p in per_file for s in p],
            "stream_file": [s[0] for s in streams], "stream_local": local,
            "pan_first": [sum(npan[:f]) for f in range(nf + 1)],
            "row_first": [sum(npan[g] * len(per_file[g]) for g in range(f)) for f in range(nf)]}


STREAM_TABLES = {
    "two files, interleaved, classes and ALL": (256, 3, [2000, 700], [[b"a", b"b", b"c"], [b"p", b"q"]],
                                                [(1, ALL, 1), (0, READ1, 2), (1, ALL, UNGROUPED), (0, READ2, 2), (0, SINGLE, UNGROUPED),
                                                 (1, ALL, 0), (0, READ1, 0)]),
    "a file without groups before one with": (256, 3, [10, 3000], [[], [b"a", b"b", b"c"]],
                                              [(1, READ2, 1), (0, ALL, UNGROUPED), (1, READ1, 1), (1, SINGLE, UNGROUPED), (1, READ1, 0)]),
    "a file without streams between two with": (64, 1, [64, 65, 0], [[b"a"], [b"a"], []],
                                                [(2, READ1, UNGROUPED), (0, ALL, 0), (2, READ2, UNGROUPED), (0, ALL, UNGROUPED)]),
    "the default segment and panel": (65536, 4, [65536 * 4 + 1, 1], [[b"a"], [b"b"]], [(1, READ1, 0), (0, READ1, 0), (0, READ2, 0)]),
}


def check_stream_tables(got, name):
    seg, panel, lengths, groups, streams = STREAM_TABLES[name]
    want = tables_want(seg, panel, lengths, streams, groups)
    assert {k: got[k] for k in want} == want
    assert got["out_offs"] == [0] * len(streams) and got["out_caps"] == [0] * len(streams)


def stream_tables_case(name):
    seg, panel, lengths, groups, streams = STREAM_TABLES[name]
    return EM.describe_case(seg, panel, lengths, streams, groups)


@pytest.mark.parametrize("name", list(STREAM_TABLES))
def test_the_map_and_the_stream_tables(name):
    check_stream_tables(EM.run(stream_tables_case(name)), name)


def test_a_text_call_states_its_slots():
    seg, panel, lengths, groups, streams = STREAM_TABLES["a file without groups before one with"]
    slots = [(16 * i, 100 + i) for i in range(len(streams))]
    got = EM.run(EM.describe_case(seg, panel, lengths, streams, groups, slots=slots))
    assert got["out_offs"] == [s[0] for s in slots] and got["out_caps"] == [s[1] for s in slots]


# ---- workspace size and descriptor block ---------------------------------------------------------------------------------
with open(os.path.join(HERE, "golden", "bam_groups_ws.json")) as _f:
    WS = json.load(_f)["rows"]


def ws_streams(row):
    """Streams of the row's files, all different: file f's j-th takes class 1 + j % 3 of group j // 3 (behind the last
    group: the ungrouped reads)."""
    seen, out = {}, []
    for f in row["stream_file"]:
        j = seen.get(f, 0)
        seen[f] = j + 1
        ng = row["groups"][f]
        assert j // 3 <= ng
        out.append((f, 1 + j % 3, UNGROUPED if j // 3 == ng else j // 3))
    return out


def align(n):
    return (n + 255) // 256 * 256


def test_the_fixture_covers_what_it_should():
    assert len(WS) >= 30
    assert {len(r["lengths"]) for r in WS} >= {0, 1, 3}
    assert {g for r in WS for g in r["groups"]} >= {0, 1, 1024}
    assert {len(r["stream_file"]) for r in WS} >= {0, 1, 40}
    assert {(r["seg_bytes"], r["panel_segs"]) for r in WS} == {(0, 0), (256, 3)}
    for seg in (256, 65536):
        assert {n for r in WS if (r["seg_bytes"] or 65536) == seg for n in r["lengths"]} >= {0, 1, seg, seg + 1}


@pytest.mark.parametrize("row", WS, ids=[r["name"] for r in WS])
def test_workspace_size_and_descriptor_block(row):
    """The size is what vk_bam_groups_workspace_size stated before the rules moved; the block's pieces lie one after
    another in bg_take's order, each at a multiple of 256 bytes, and the pieces behind the block add up to the size."""
    seg, panel = row["seg_bytes"] or 65536, row["panel_segs"] or 4
    groups = [names(n) for n in row["groups"]]
    streams = ws_streams(row)
    got = EM.run(EM.describe_case(seg, panel, row["lengths"], streams, groups))
    assert got["workspace"] == row["bytes"]
    at = 0
    for name, size in EM.PIECES:
        assert got["at"][name] == at, name
        at += align(len(got[name]) * size)
    assert got["desc_bytes"] == at
    nf, ns = len(row["lengths"]), len(streams)
    assert got["back_bytes"] == align(4 * nf) + align(8)
    nseg = [max(1, -(-n // seg)) for n in row["lengths"]]
    rows = sum(-(-nseg[f] // panel) * row["stream_file"].count(f) for f in range(nf))
    scap = seg // 37 + 2
    assert got["workspace"] == at + got["back_bytes"] + align(2 * sum(nseg) * scap) + align(16 * rows) + align(16 * ns)
    want = tables_want(seg, panel, row["lengths"], streams, groups)
    assert {k: got[k] for k in want} == want
    assert got["ids"] == list(b"".join(i for g in groups for i in g)) and got["group_first"] == [sum(row["groups"][:f]) for f in range(nf + 1)]


# ---- result rules ------------------------------------------------------------------------------------------------------
RESULTS = {
    "pick ALL": (EM.pick_case([5, 7, 11], ALL), 23),
    "pick READ1": (EM.pick_case([5, 7, 11], READ1), 5),
    "pick READ2": (EM.pick_case([5, 7, 11], READ2), 7),
    "pick SINGLE": (EM.pick_case([5, 7, 11], SINGLE), 11),
    "pick ALL past 2^32": (EM.pick_case([1 << 33, 1 << 33, 1], ALL), (1 << 34) + 1),
    "a sound file": (EM.status_case(0, 0), 0),
    "a sound file whose aux was bad": (EM.status_case(0, 1), BAD_AUX),
    "a file's own status comes first": (EM.status_case(TRUNCATED, 1), TRUNCATED),
    "a file's own status": (EM.status_case(BAD_RECORD, 0), BAD_RECORD),
    "a text that fills its slot": (EM.slot_case(4096, 4096), {"fits": True, "length": 4096}),
    "a text one byte too long": (EM.slot_case(4097, 4096), {"fits": False, "length": 0}),
    "no text in no room": (EM.slot_case(0, 0), {"fits": True, "length": 0}),
    "a byte in no room": (EM.slot_case(1, 0), {"fits": False, "length": 0}),
}


@pytest.mark.parametrize("name", list(RESULTS))
def test_result_rules(name):
    case, want = RESULTS[name]
    assert EM.run(case) == want


# ---- the same under the sanitizers ------------------------------------------------------------------------------------------
def test_the_same_cases_under_the_sanitizers(tmp_path):
    """The refusal, limit, table, stream-table and result cases through the stand-alone program built with
    -fsanitize=address,undefined: every array a rule reads, and every piece of the table the probe reads, is as long as
    the case says and no longer."""
    exe = EM.sanitizer_program(str(tmp_path))
    cases = ([c for c, _, _ in ARGS.values()] + [c for c, _ in PLANS.values()] + [c for c, _ in TABLES.values()] +
             [stream_tables_case(n) for n in STREAM_TABLES] + [c for c, _ in RESULTS.values()])
    got = iter(EM.run_program(exe, cases, str(tmp_path)))
    for _, bam_ok, bg_ok in ARGS.values():
        assert next(got) == {"bam_args_ok": bam_ok, "bg_args_ok": bg_ok}
    for _, want in PLANS.values():
        assert next(got) == want
    for _, nids in TABLES.values():
        check_table(next(got), nids)
    for name in STREAM_TABLES:
        check_stream_tables(next(got), name)
    for _, want in RESULTS.values():
        assert next(got) == want
