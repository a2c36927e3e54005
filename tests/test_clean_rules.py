"""Step B (`image --from-raw`) on the CPU: the cleaning rules as tests/clean_ref.py restates them, at every boundary;
the host half (inputs, R1/R2 pairing, read budget) against the reference's own functions
(tests/golden/raw_input_cases.json, written by tools/gen_raw_input_golden.py); the CLI's new flag; and that the edge
batches of tests/clean_cases.py hit what they are built to hit."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_cases as K  # noqa: E402
import clean_ref as R  # noqa: E402

from varkoder_amd import cli, rawinput  # noqa: E402

GOLDEN = json.loads((Path(__file__).parent / "golden" / "raw_input_cases.json").read_text())


def seqs(text):
    lines = text.split(b"\n")
    return {lines[i][1:].split(b" ")[0]: lines[i + 1] for i in range(0, len(lines) - 1, 4)}


def run(case, **kw):
    c = R.hand_cases()[case]
    return R.clean_sample(c["r1"], c["r2"], c["singles"], F=c["F"], T=c["T"], **kw)


def test_poly_g_boundaries():
    got = {k: len(v) for k, v in seqs(run("poly_g")[0]).items()}
    # runs of 7, 8 stay; 9 and 10 go (the loop reaches i = 10 once two non-G follow a run of 9)
    assert got[b"g7"] == 27 and got[b"g8"] == 28 and got[b"g9"] == 20 and got[b"g10"] == 20
    # one mismatch per 8 bases is allowed all the way; two before position 9 end the scan early
    assert got[b"every8"] == 20 and got[b"two_early"] == 40
    # 5 mismatches are allowed, the 6th ends the scan at the last G before it
    assert got[b"mism5"] == 20 and got[b"mism6"] == 80 - 47
    assert b"allG" not in got and b"empty" not in got and got[b"short"] == 3


def test_poly_g_loop_literal():
    assert R.poly_g(b"") == 0 and R.poly_g(b"G" * 9) == 9 and R.poly_g(b"G" * 10) == 0
    assert R.poly_g(b"ACGT" * 5 + b"G" * 10) == 18


def test_overlap_30_and_31():
    c = R.hand_cases()["overlap_lengths"]
    by = {a[0][1:].split(b" ")[0]: (a[1], b[1]) for a, b in zip(c["r1"], c["r2"])}
    assert R.overlap(*by[b"ins169"])[1] == 31     # 2 x 100 - 169
    assert R.overlap(*by[b"ins170"]) is None      # ol = 30: the forward loop stops before it
    got = seqs(run("overlap_lengths", adapter=False)[0])
    assert len(got[b"ins169"]) == 169 and len(got[b"ins200"]) == 100


def test_mismatch_limit_inside_and_past_50():
    text, st = run("mismatch_limit")
    names = [ln for ln in text.split(b"\n")[::4] if ln]
    assert sum(n.startswith(b"@m5") for n in names) == 1      # merged: 5 <= min(5, 100 // 5)
    assert sum(n.startswith(b"@m6") for n in names) == 2      # 6 > 5: two records
    assert sum(n.startswith(b"@late10") for n in names) == 1  # past position 50 nothing is counted
    merged = seqs(text)[b"m5"]
    c = R.hand_cases()["mismatch_limit"]
    assert merged[:150] == c["r1"][0][1] and len(merged) == 200   # R1's bases win in the overlap


def test_readthrough_adapter():
    c = R.hand_cases()["readthrough_F0"]
    ins = c["r1"][0][1][:120]
    assert R.overlap(c["r1"][0][1], c["r2"][0][1]) == (-30, 120)
    assert seqs(run("readthrough_F0")[0])[b"rt"] == ins
    text, _ = run("readthrough_F0", merge=False)      # adapters cut, pair kept as two records
    lines = text.split(b"\n")
    assert lines[1] == ins and lines[5] == R.revcomp(ins)
    for case in ("readthrough_F10", "readthrough_F7_T3"):
        got = seqs(run(case)[0])[b"rt"]
        assert got in ins and len(got) >= 90
    text, _ = run("readthrough_F0", adapter=False, merge=False)
    assert text.split(b"\n")[1] == c["r1"][0][1]       # -a -r: nothing is cut


def test_trim_front_tail_bounds():
    text, st = run("trim_bounds")
    got = seqs(text)
    assert b"l19" not in got and b"l20" not in got and got[b"l21"] == R.hand_cases()["trim_bounds"]["singles"][2][1][10:11]
    assert b"p19" not in got    # F + T > len(R1): the whole pair goes
    assert st["records"] == 1 and st["clean_bp"] == 1
    # without merging, a pair whose R1 trims to nothing still writes its R2
    assert b"p20" in seqs(run("trim_bounds", merge=False)[0])


def test_duplicates_se_and_pe():
    text, st = run("duplicates")
    names = [ln[1:] for ln in text.split(b"\n")[::4] if ln]
    assert names == [b"x", b"x", b"y", b"y", b"z", b"z", b"a", b"b", b"c"]   # pairs (unmerged: two records) first, then singles
    _, st2 = run("duplicates", dedup=False)
    assert st2["records"] == st["records"] + 3     # one pair (two records) and one single were duplicates


@pytest.mark.parametrize("adapter", [True, False])
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("dedup", [True, False])
def test_flag_combinations(adapter, merge, dedup):
    r1, r2, singles = R.synth_set(5, 300, 100)
    text, st = R.clean_sample(r1, r2, singles, adapter=adapter, merge=merge, dedup=dedup)
    recs = R.parse_fastq(text)
    assert recs is not None and len(recs) == st["records"] and all(s for _, s, _ in recs)
    assert st["clean_bp"] == sum(len(s) for _, s, _ in recs)
    merged = sum(1 for h, _, _ in recs if h.endswith(b" 1:N:0")) - sum(1 for h, _, _ in recs if h.endswith(b" 2:N:0"))
    assert (merged > 0) == merge
    dups = sum(1 for h, _, _ in recs if h.startswith(b"@dup") or h.startswith(b"@sdup"))
    assert (dups == 0) == dedup
    if not adapter and not merge:
        assert max(len(s) for h, s, _ in recs if h.endswith(b":N:0")) == 130   # 150 - 10 - 10, nothing cut


def test_base_counts_first_group():
    c = R.hand_cases()["readthrough_F0"]
    _, st = R.clean_sample(c["r1"], c["r2"], [(b"@s", b"T" * 50, b"I" * 50)], F=0, T=0)
    assert st["reach"][:40] == [1] * 40             # the merged read only: singles are not the first group
    ins = c["r1"][0][1]
    for i in range(40):
        assert st["base"][i][b"ACGT".index(ins[i:i + 1])] == 1
    curves = rawinput.content_curves(st["base"], st["reach"])
    assert set(curves) == set("ATCG") and len(curves["A"]) == 40
    assert rawinput.curves_sd(curves) > 0.3


def test_parse_fastq_framing():
    good = R.fq([(b"@a", b"ACGT", b"IIII"), (b"@b", b"AC", b"II")])
    assert len(R.parse_fastq(good)) == 2 and len(R.parse_fastq(good[:-1])) == 1   # newlines // 4
    assert R.parse_fastq(good, 3) is None
    assert R.parse_fastq(good.replace(b"@b", b"b@")) is None
    assert R.parse_fastq(good.replace(b"IIII", b"III")) is None


# ------------------------------------------------- the edge batches (clean_cases) ---
# What each builder is meant to hit, shown on the reference side: the GPU tests (test_gpu_clean_edges.py) then hold the
# kernels to the same batches.

def test_budget_batch_hits_its_cases():
    b = K.budgets()
    want = K.expected(b)
    names = b["names"]
    assert [w[2] for w in want] == [K.RAGGED if j == names["ragged"] else 0 for j in range(b["nsamples"])]
    files = lambda j: [i for i in range(len(b["owner"])) if b["owner"][i] == j]
    held = lambda i: b["texts"][i].count(b"\n") // 4
    # crossed: unequal files, equal budgets, the R1 / R2 file boundary at different pairs; a middle file that gives none
    r1 = [i for i in files(names["crossed"]) if b["roles"][i] == K.R1]
    r2 = [i for i in files(names["crossed"]) if b["roles"][i] == K.R2]
    se = [i for i in files(names["crossed"]) if b["roles"][i] == K.SE]
    assert len(r1) == len(r2) == 2 and len(se) == 3
    assert sum(b["records"][i] for i in r1) == sum(b["records"][i] for i in r2) == 400
    assert b["records"][r1[0]] != b["records"][r2[0]] and sum(map(held, r1)) != sum(map(held, r2))
    assert b["records"][se[1]] == 0 and held(se[1]) > 0 and b["records"][se[0]] and b["records"][se[2]]
    assert sum(b["records"][i] < held(i) for i in r1 + r2 + se) >= 5
    g = K.groups(b)[names["crossed"]]
    assert [h.split(b" ")[0] for h, _, _ in g[0]] == [h.split(b" ")[0] for h, _, _ in g[1]]   # mates meet
    assert want[names["crossed"]][0] and not any(b"extra" in ln for ln in want[names["crossed"]][0].split(b"\n")[::4])
    # every budget 0: nothing out, no status, no stats
    assert all(b["records"][i] == 0 and held(i) for i in files(names["all_zero"]))
    assert want[names["all_zero"]] == (b"", [0] * K.NSTAT, 0)
    assert [b["records"][i] for i in files(names["one"])] == [1] and want[names["one"]][1][1] == 1
    # a budget that ends with byte 16383 of its file, and one a record later
    for tag, more in (("at", 0), ("past", 1)):
        i, n = b["chunk_files"][tag]
        text = b["texts"][i]
        assert b["records"][i] == n + more < held(i)
        assert len(b"\n".join(text.split(b"\n")[:4 * n]) + b"\n") == K.CHUNK and text[K.CHUNK - 1:K.CHUNK] == b"\n"
    # garbage behind the budget: status 0 as budgeted, bad framing as a whole file
    i = names["garbage_file"]
    assert R.parse_fastq(b["texts"][i], b["records"][i]) is not None and R.parse_fastq(b["texts"][i]) is None
    assert want[names["garbage"]][2] == 0 and want[names["garbage"]][0]
    for bad in (K.GARBAGE[:23], K.GARBAGE[23:51], K.GARBAGE[51:]):     # each record of it is bad in its own way
        assert bad.count(b"\n") == 4 and R.parse_fastq(bad) is None
    # ragged by budget alone
    i, j = files(names["ragged"])
    assert held(i) == held(j) and b["records"][i] != b["records"][j]
    whole = dict(b, records=[held(i) for i in range(len(b["texts"]))])
    assert K.groups(whole)[names["ragged"]][3] == 0


def test_file_end_batch_hits_its_cases():
    b = K.file_ends()
    lens = [len(t) for t in b["texts"]]
    assert {n % 64 for n in lens[:64]} == set(range(64))
    assert [lens[b["sized"][n]] for n in (16383, 16384, 16385)] == [16383, 16384, 16385]
    i = b["unterminated"]
    assert not b["texts"][i].endswith(b"\n") and b["records"][i] == (b["texts"][i] + b"\n").count(b"\n") // 4 - 1
    assert lens[b["empty"]] == 0 and 0 in lens[b["empty"] + 1:]
    for text, slack in zip(b["texts"], b["slack"]):
        assert len(slack) >= 80 and len(R.parse_fastq(slack)) * 4 == slack.count(b"\n") >= 56
        assert b"\n" in slack[:4 - len(text) % 4] or len(text) % 4 in (0, 3)   # a newline in the end's own word
    want = K.expected(b, F=0, T=0)
    assert not any(w[2] for w in want) and sum(1 for w in want if w[0]) == b["nsamples"] - 1
    assert want[b["owner"][b["empty"]]] == (b"", [0] * K.NSTAT, 0)


def test_long_line_batch_hits_its_cases():
    b = K.long_lines()
    lines = b["texts"][0].split(b"\n")
    assert max(map(len, lines)) == 40000 and sorted(map(len, lines))[-3] == 20000
    assert b"\n" not in b["texts"][0][3 * K.CHUNK:4 * K.CHUNK]            # a chunk without a newline
    want = K.expected(b)
    assert not any(w[2] for w in want)
    assert max(map(len, want[0][0].split(b"\n"))) == 40000 - 20
    merged = [ln for ln in want[1][0].split(b"\n") if len(ln) > 20000]
    assert len(merged) == 2 and len(merged[0]) == 31000 - 20               # the mates overlap: one read of the insert


def test_many_small_batch_hits_its_cases():
    b = K.many_small()
    assert b["nsamples"] == 300 and len(b["texts"]) > 300
    g = K.groups(b)
    units = [len(r1) + len(se) for r1, _, se, _ in g]
    assert units == [K.UNIT_CYCLE[j % 11] for j in range(300)]
    kinds = {(bool(r1), bool(se)) for r1, _, se, _ in g}
    assert kinds == {(True, False), (False, True), (True, True), (False, False)}
    starts = np.cumsum([0] + units[:-1])
    assert len({int(s) % 64 for s in starts}) > 48 and len({int(s) % 256 for s in starts}) > 100
    assert {int(s) % 64 for s in starts} >= {0, 1, 15, 16, 17, 63}         # wavefront and workgroup edges
    want = K.expected(b)
    assert not any(w[2] for w in want)
    assert sum(1 for w in want if w[1][1]) > 250
    import adapter_ref as A
    ads = [A.clean_sample_adapters(r1, r2, se, adapters=t)[2] for (r1, r2, se, _), t in zip(g, b["adapters"])]
    assert sum(1 for a in ads if a["reads"]) > 150                        # trimming by sequence has work all over


@pytest.mark.parametrize("F,T", K.TRIMS)
def test_dirty_pair_batch_hits_its_cases(F, T):
    b = K.dirty_pairs(F, T)
    r1, r2 = b["pairs"]
    assert 2900 <= len(r1) == len(r2) <= 3100
    kept = {(len(a[1]) - F - T, len(c[1]) - F - T) for a, c in zip(r1, r2)}
    for k in K.KEPT:
        assert any(x == k for x, _ in kept) and any(y == k for _, y in kept), k
    assert any(x <= 1 and y == 150 for x, y in kept) and any(y <= 1 and x == 150 for x, y in kept)
    outcomes = [K.outcome(a, c, F, T) for a, c in zip(r1, r2)]
    count = {o: outcomes.count(o) for o in set(outcomes)}
    assert set(count) == {"merged", "cut", "unmerged", "dropped"} and min(count.values()) >= 50, count
    # the planted mismatches decide: 4 and 5 merge, 6 do not; an equal N costs nothing, an unequal byte one mismatch
    by = {}
    for a, o in zip(r1, outcomes):
        if a[0].startswith(b"@m"):
            m, f = int(a[0][2:3]), int(a[0][5:6])
            by.setdefault((m, f), []).append(o in ("merged", "cut"))
    assert len(by) == 12 and all(len(v) >= 30 for v in by.values())
    for (m, f), v in by.items():
        assert all(v) == (m + (f >= 2) <= 5) and any(v) == all(v), (m, f)
    seqs = [(a[1], c[1]) for a, c in zip(r1, r2)]
    assert 200 <= len(seqs) - len(set(seqs)) <= 400                        # exact duplicates
    assert 200 <= sum(1 for a in r1 if a[0].startswith(b"@r2only")) <= 400
    every = b"".join(a[1] + c[1] for a, c in zip(r1, r2))
    assert all(ch in every for ch in b"NnacgtRY.-")


def test_framing_batch_is_well_formed():
    b = K.framing()
    assert b["texts"][0].count(b"\r\n") == b["texts"][0].count(b"\n") and b["roles"][:3] == [K.SE, K.R1, K.R2]
    for text in b["texts"][3:]:
        lines = text.split(b"\n")
        assert any(p.startswith(b"+") and len(p) > 1 for p in lines[2::4])
        assert b"@" in lines[0::4] and b"" in lines[1::4]
        assert any(q.startswith(b"@") for q in lines[3::4]) and any(q.startswith(b"+") for q in lines[3::4])
    want = K.expected(b)
    assert not any(w[2] for w in want) and all(w[0] for w in want)
    assert b"\r\n+\n" in K.expected(b, F=0, T=0)[0][0]                     # the '\r' is a byte of the sequence line
    assert all(ln == b"+" for w in want for ln in w[0].split(b"\n")[2::4])


def test_big_identity_closed_form():
    b = K.big_identity()
    assert b["records"][0] > 1 << 20 and len(b["texts"][0]) == 62 * b["records"][0]
    text, words = b["closed"][0](0, 0, True, True, True)
    assert text is b["texts"][0] and words[:2] == [24 * b["records"][0], b["records"][0]]
    n = 2000
    small = K.big_identity(n)
    for i in range(0, n, 97):                                            # the same headers and ordinals
        assert small["texts"][0][62 * i:62 * i + 24] == b["texts"][0][62 * i:62 * i + 24]
    recs = R.parse_fastq(small["texts"][0])
    assert len(recs) == n and len({s for _, s, _ in recs}) == n and not any(b"G" in s for _, s, _ in recs)
    for flags in ((True, True, True), (False, False, False)):
        got, st = R.clean_sample([], [], recs, 0, 0, *flags)
        assert (got, K.stats_words(st)) == small["closed"][0](0, 0, *flags)



def test_process_input_folder(tmp_path):
    root = tmp_path / "input"
    for d, files in GOLDEN["tree"].items():
        (root / d).mkdir(parents=True)
        for f in files:
            (root / d / f).write_bytes(b"")
    for f in GOLDEN["loose"]:
        (root / f).write_bytes(b"")
    got = [[s, lab, [str(Path(f).relative_to(root)) for f in files]] for s, lab, files in rawinput.process_input(root)]
    assert got == GOLDEN["folder"]


def test_process_input_csv(tmp_path):
    csv = tmp_path / "table" / "samples.csv"
    csv.parent.mkdir()
    csv.write_text(GOLDEN["csv_text"])
    got = [[s, lab, [str(Path(f).relative_to(csv.parent)) for f in files]] for s, lab, files in rawinput.process_input(csv)]
    assert got == GOLDEN["csv"]


@pytest.mark.parametrize("name", sorted(GOLDEN["pairing"]))
def test_pairing_matches_reference(name):
    case = GOLDEN["pairing"][name]
    assert rawinput.pair_files(case["files"]) == case["reads"]


def test_pairing_keeps_the_reference_quirk():
    """Two mateless R1 in a row: the second stays in R1 (the reference deletes from the list it walks)."""
    got = rawinput.pair_files(["a_1.fq", "b_1.fq", "c_1.fq", "c_2.fq"])
    assert got == {"R1": ["b_1.fq", "c_1.fq"], "R2": ["c_2.fq"], "unpaired": ["a_1.fq"]}


@pytest.mark.parametrize("i", range(len(GOLDEN["budget"])))
def test_read_budget_matches_reference(i):
    case = GOLDEN["budget"][i]
    assert rawinput.reads_needed(case["files_info"], case["max_bp"]) == case["take"]


def test_avg_read_length():
    text = R.fq([(b"@r%d" % i, b"A" * (100 + i % 3), b"I" * (100 + i % 3)) for i in range(12000)])
    want = sum(100 + i % 3 for i in range(10000)) / 10000
    assert rawinput.avg_read_length(text) == want


# ---------------------------------------------------------------------- CLI ---

def test_cli_refuses_raw_and_clean(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        cli.setup_parser().parse_args(["image", str(tmp_path), "--from-raw", "--from-clean"])
    assert e.value.code == 2
    assert "not allowed with" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["image", "in"], ["image", "in", "--from-clean", "-a", "-D", "-r", "-T", "5,5"],
                                  ["image", "in", "-k", "9", "-M", "0", "-i", "int", "-x"]])
def test_parser_without_from_raw_is_unchanged(argv):
    ns = vars(cli.setup_parser().parse_args(argv))
    assert ns.pop("from_raw") is False
    want = {"command": "image", "input": "in", "seed": None, "overwrite": False, "verbose": False, "kmer_size": 7,
            "kmer_mapping": "cgr", "n_threads": 1, "cpus_per_thread": 1, "outdir": "images", "stats_file": "stats.csv",
            "int_folder": None, "min_bp": "500K", "max_bp": "200M", "label_table": False, "no_adapter": False,
            "no_deduplicate": False, "no_merge": False, "no_image": False, "trim_bp": "10,10", "labels_csv": None,
            "from_clean": False}
    extra = argv[2:]
    if "--from-clean" in extra:
        want.update(from_clean=True, no_adapter=True, no_deduplicate=True, no_merge=True, trim_bp="5,5")
    if "-k" in extra:
        want.update(kmer_size=9, max_bp="0", int_folder="int", overwrite=True)
    assert ns == want
    assert cli.setup_parser().parse_args(["image", "in", "--from-raw"]).from_raw is True
