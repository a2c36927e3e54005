"""The host rules of the FASTA calls (csrc/vk_faplan.h) on a CPU, through tests/emul/faplan_emul.cpp: the unit override, the
plan and the pair table word for word against a restatement in Python (faplan_emul_lib.py, written from the comment at the
head of csrc/vk_fasta.h), what the plan, the pair rules, rec_first and the window rules refuse and the neighbour they accept,
the refusal table of the six entry points, the four layouts' pieces -- and the same cases through the sanitizer build."""
import pytest

import faplan_emul_lib as EM
from faplan_emul_lib import (ACCEPTED, COUNT_RECORDS, COUNT_WINDOWS, L_COUNT, L_RECORDS, L_SAMPLED, L_STATE, L_WINDOWS, OFFSETS_STAGE,
                             PLAN_STAGE, RULES_STAGE, VK_EINVAL, VK_OK)

# ---- the unit override ---------------------------------------------------------------------------------------------------
CLAMPS = {0: 0, 1: 64, 63: 64, 64: 64, 65: 64, 256: 256, 16384: 16384, 16385: 16384, 2 ** 32 - 1: 16384}


def test_unit_override():
    for env, want in CLAMPS.items():
        assert EM.clamp_ref(env) == want
        assert EM.run(EM.clamp_case(env)) == want, env


# ---- the plan ----------------------------------------------------------------------------------------------------------------
OVERRIDES = (0, 64, 256, 16384)


def plan_lengths(override):
    """0 and 1, around a unit and around a workgroup's span of units."""
    unit, span = (override, 1) if override else (EM.UNIT, EM.SPAN)
    return sorted({0, 1, unit - 1, unit, unit + 1, span * unit - 1, span * unit, span * unit + 1})


def plan_cases():
    cases = []
    for ov in OVERRIDES:
        one = plan_lengths(ov)
        cases += [(ov, [16 * i], [x]) for i, x in enumerate(one)]
        mixed = one[2:5] + [0] + one[5:] + one[:2]   # (an empty sample in the middle)
        cases.append((ov, [32 * i for i in range(len(mixed))], mixed))
    cases.append((0, [], []))
    return cases


PLAN_CASES = plan_cases()


def test_the_plan_cases_cover_what_they_should():
    for ov in OVERRIDES:
        mine = [c for c in PLAN_CASES if c[0] == ov]
        assert {x for c in mine if len(c[2]) == 1 for x in c[2]} == set(plan_lengths(ov))
        assert any(len(c[2]) > 3 and 0 in c[2][1:-1] for c in mine)
    want = EM.plan_ref(0, [0, 16], [EM.UNIT * EM.SPAN + 1, 1])   # the restatement itself, on numbers written out
    assert want == {"status": 0, "unit": 16384, "span": 32, "nwg": 3, "nunits": 34,
                    "meta": [0, 16, 524289, 1, 0, 2, 3, 0, 33, 34]}


@pytest.mark.parametrize("case", PLAN_CASES, ids=[f"{c[0]}-{'+'.join(map(str, c[2]))}" for c in PLAN_CASES])
def test_plan(case):
    assert EM.run(EM.plan_case(*case)) == EM.plan_ref(*case)


BIG = EM.BIG
PLAN_REFUSALS = [
    ("the first offset off 16 bytes", (0, [8, 64], [40, 50]), VK_EINVAL),
    ("the last offset off 16 bytes", (0, [0, 72], [40, 50]), VK_EINVAL),
    ("offsets at 16 bytes", (0, [16, 80], [40, 50]), VK_OK),
    ("a sample of 2^30 units", (0, [0], [2 ** 30 * EM.UNIT]), VK_EINVAL),
    ("a sample of 2^30 - 1 units", (0, [0], [BIG * EM.UNIT]), VK_OK),
    ("a sample of 2^30 units of 64 bytes", (64, [0], [2 ** 30 * 64]), VK_EINVAL),
    ("a sample of 2^30 - 1 units of 64 bytes", (64, [0], [BIG * 64]), VK_OK),
    ("three samples of 2^30 - 1 units of 64 bytes", (64, [0, 0, 0], [BIG * 64] * 3), VK_EINVAL),
    ("two samples of 2^30 - 1 units of 64 bytes", (64, [0, 0], [BIG * 64] * 2), VK_OK),
]


@pytest.mark.parametrize("name", [r[0] for r in PLAN_REFUSALS])
def test_plan_refusals(name):
    """Numbers only: no text of that size exists."""
    _, case, status = next(r for r in PLAN_REFUSALS if r[0] == name)
    got, want = EM.run(EM.plan_case(*case)), EM.plan_ref(*case)
    assert want["status"] == status and got == want


# ---- the pair plan -----------------------------------------------------------------------------------------------------------
# three samples of 3, 0 and 1 workgroups (full units) or 65, 0 and 1 (units of 256 bytes); a sample named twice, one not at all
PAIR_BATCH = ([0, 16384 * 80, 16384 * 80], [EM.UNIT * EM.SPAN * 2 + 5, 0, 700])
PAIR_CASES = [(ov, PAIR_BATCH[0], PAIR_BATCH[1] if ov == 0 else [256 * 64 + 5, 0, 200], pairs)
              for ov in (0, 256)
              for pairs in ([], [(2, 11, 2 ** 32, 2 ** 63 - 1)], [(0, 7, 0, 0), (2, 8, 5, 1), (0, 9, 2 ** 31, 77), (1, 1, 1, 1)])]


def test_pair_plan():
    for case in PAIR_CASES:
        plan = EM.plan_ref(*case[:3])
        want = EM.pairs_ref(plan, case[3])
        assert EM.run(EM.pairs_case(*case)) == want, case
    plan = EM.plan_ref(*PAIR_CASES[2][:3])
    assert EM.pairs_ref(plan, PAIR_CASES[2][3])["words"][-5:] == [0, 3, 4, 7, 7]   # (the restatement, on numbers written out)
    assert EM.pairs_ref(plan, [])["words"] == [0]


# ---- rec_first -----------------------------------------------------------------------------------------------------------------
FIRSTS = [([0, 1, 2], True), ([1, 1, 2], False), ([0, 2, 1], False), ([0, 1, 1], True), ([0, 0, 0], True), ([0], True), ([1], False)]


def test_rec_first():
    for rec_first, ok in FIRSTS:
        assert EM.run(EM.first_case(rec_first)) is ok, rec_first


# ---- the refusal table -----------------------------------------------------------------------------------------------------
def refusal_case(r):
    args = {k: v for k, v in r["args"].items() if k != "text"}
    return EM.check_case(r["call"], **args)


def header_rows():
    """The rows the header can answer: it never sees d_fasta."""
    return [r for r in EM.REFUSALS if r["args"].get("text", "ok") == "ok"]


def test_the_refusal_table_covers_what_it_should():
    names = [r["name"] for r in EM.REFUSALS]
    assert len(set(names)) == len(names)
    for call in range(len(EM.ENTRY_POINTS)):   # every entry point has rows, refused and accepted, on the CPU and for the GPU
        mine = [r for r in EM.REFUSALS if r["call"] == call]
        assert {r["status"] for r in mine} == {VK_OK, VK_EINVAL}
        assert {r["status"] for r in mine if r["gpu"]} == {VK_OK, VK_EINVAL}
        assert {r["rule"] for r in mine} >= {"none", "offset", "2^30 units", "2^31 workgroups", "no sample", "d_fasta"}
    assert {r["rule"] for r in EM.REFUSALS} == set(EM.RULES)   # every rule has a row ...
    for rule in set(EM.RULES) - {"none", "no sample", "d_fasta"}:   # ... a refusal and the accepted edge beside it
        assert {r["status"] for r in EM.REFUSALS if r["rule"] == rule} == {VK_OK, VK_EINVAL}, rule
    # what reaches an entry point returns before a launch: a refusal, or a batch without a sample
    assert all(r["status"] != VK_OK or not r["args"]["offsets"] for r in EM.REFUSALS if r["gpu"])
    # the wart: the two per-row counting calls reset d_hist ahead of the plan's refusals and of the answer to no sample, and
    # behind the offsets' -- and the GPU test gives them one row at k = 5 to reset
    for r in EM.REFUSALS:
        if r["resets"]:
            a = r["args"]
            assert r["call"] in (COUNT_RECORDS, COUNT_WINDOWS) and r["gpu"] and (a["k"], a["nslots"], a["nrows"]) == (5, 1, 1)
            assert r["stage"] == (PLAN_STAGE if r["status"] else ACCEPTED)
        elif r["gpu"] and r["call"] in (COUNT_RECORDS, COUNT_WINDOWS):
            assert r["status"] == VK_EINVAL and r["stage"] in (RULES_STAGE, OFFSETS_STAGE)
    assert any(r["resets"] and r["status"] for r in EM.REFUSALS) and any(r["resets"] and not r["status"] for r in EM.REFUSALS)
    assert sum(r["gpu"] for r in EM.REFUSALS) >= 90


@pytest.mark.parametrize("name", [r["name"] for r in header_rows()])
def test_refusals(name):
    r = next(r for r in EM.REFUSALS if r["name"] == name)
    got = EM.run(refusal_case(r))
    assert (got["status"], got["stage"]) == (r["status"], r["stage"])


def test_window_numbers():
    """steps and sum_wgs go back to the caller: tiles of a window, and tile rows times chunks of 1024 codes."""
    win = lambda **k: EM.run(EM.check_case(COUNT_WINDOWS, offsets=[0], lengths=[100], **k))   # noqa: E731
    assert win(k=7, win_len=700, win_step=100, tile_rows=3) == {"status": 0, "stage": ACCEPTED, "steps": 7, "sum_wgs": 3 * (4 ** 7 // EM.SUM_CODES)}
    assert win(k=9, win_len=64 * 9, win_step=9, tile_rows=10) == {"status": 0, "stage": ACCEPTED, "steps": 64, "sum_wgs": 10 * (4 ** 9 // EM.SUM_CODES)}
    assert win(k=5, win_len=100, win_step=100, tile_rows=10) == {"status": 0, "stage": ACCEPTED, "steps": 1, "sum_wgs": 0}


# ---- the four layouts ----------------------------------------------------------------------------------------------------
LAYOUT_LENGTHS = ([], [0], [1], [63, 0, 16385], [16384 * 32 + 1, 700])
LAYOUT_CASES = [(fn, ov, lengths, extra)
                for ov in (0, 256)
                for lengths in LAYOUT_LENGTHS
                for fn, extras in ((L_COUNT, [{}]), (L_STATE, [{}]), (L_RECORDS, [{}]),
                                   (L_SAMPLED, [dict(npairs=0), dict(npairs=7)]),
                                   (L_WINDOWS, [dict(total=0, steps=1, tile_rows=5, k=7), dict(total=9, steps=2, tile_rows=5, k=7),
                                                dict(total=40, steps=64, tile_rows=1, k=5)]))
                for extra in extras]


def check_layout(got, case):
    fn, ov, lengths, extra = case
    total, pieces = EM.layout_ref(fn, ov, lengths, **extra)
    assert got["total"] == total and got["pieces"] == [(off, size) for _, off, size in pieces], [p[0] for p in pieces]


def test_the_layout_restatement():
    """On numbers written out: two samples of 33 and 1 full units; units of 256 bytes are four lanes each."""
    total, pieces = EM.layout_ref(L_SAMPLED, 0, [16384 * 32 + 1, 700], npairs=7)
    assert pieces == [("meta", 0, 80), ("pairs", 256, 288), ("ukey", 768, 140), ("carry", 1024, 140), ("unit_ord", 1280, 280),
                      ("lane", 1792, 4 * (34 * 256 + 1))] and total == 1792 + 34816 + 256
    _, pieces = EM.layout_ref(L_WINDOWS, 256, [700], total=9, steps=2, tile_rows=5, k=7)
    assert pieces == [("lane", 0, 52), ("unit_ord", 256, 32), ("bases", 512, 8), ("recs", 768, 240), ("used", 1024, 4),
                      ("tiles", 1280, 5 * 16384 * 4)]
    assert EM.layout_ref(L_WINDOWS, 256, [700], total=9, steps=1, tile_rows=5, k=7)[1][-1] == ("tiles", 1280, 4)
    # a caller's workspace counts a unit per lane, whatever the switch says
    assert EM.layout_ref(L_STATE, 0, [700])[1] == EM.layout_ref(L_STATE, 256, [700])[1] == [("meta", 0, 48), ("ukey", 256, 48),
                                                                                          ("carry", 512, 48)]
    assert EM.layout_ref(L_COUNT, 0, [700])[1] == [("meta", 0, 48), ("ukey", 256, 8), ("carry", 512, 8)]


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=[f"{c[0]}-{c[1]}-{'+'.join(map(str, c[2]))}-{i}" for i, c in enumerate(LAYOUT_CASES)])
def test_layouts(case):
    fn, ov, lengths, extra = case
    check_layout(EM.run(EM.layout_case(fn, ov, lengths, **extra)), case)


# ---- the same under the sanitizers ------------------------------------------------------------------------------------------
def test_the_same_cases_under_the_sanitizers(tmp_path):
    """Every case above through the stand-alone program built with -fsanitize=address,undefined: every array a rule reads is
    as long as the case says and no longer, and every piece of a layout lies inside a block of exactly the layout's size."""
    exe = EM.sanitizer_program(str(tmp_path))
    rows = header_rows()
    cases = ([EM.clamp_case(e) for e in CLAMPS] + [EM.plan_case(*c) for c in PLAN_CASES] + [EM.plan_case(*r[1]) for r in PLAN_REFUSALS]
             + [EM.pairs_case(*c) for c in PAIR_CASES] + [EM.first_case(f) for f, _ in FIRSTS] + [refusal_case(r) for r in rows]
             + [EM.layout_case(c[0], c[1], c[2], **c[3]) for c in LAYOUT_CASES])
    got = iter(EM.run_program(exe, cases, str(tmp_path)))
    for want in CLAMPS.values():
        assert next(got) == want
    for c in PLAN_CASES:
        assert next(got) == EM.plan_ref(*c)
    for r in PLAN_REFUSALS:
        assert next(got) == EM.plan_ref(*r[1])
    for c in PAIR_CASES:
        assert next(got) == EM.pairs_ref(EM.plan_ref(*c[:3]), c[3])
    for _, ok in FIRSTS:
        assert next(got) is ok
    for r in rows:
        g = next(got)
        assert (g["status"], g["stage"]) == (r["status"], r["stage"]), r["name"]
    for c in LAYOUT_CASES:
        check_layout(next(got), c)
