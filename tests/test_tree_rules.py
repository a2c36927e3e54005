"""The rule of `tree` without a GPU: the two statements of tests/tree_ref.py agree bit for bit; additive trees come back with
their splits and edge lengths; ties join in the order the rule says; Newick round-trips awkward names;
--no-negative-branches keeps a pair's path length; the vectorised distances of sketch.py equal the scalar ones exactly;
Jukes-Cantor and every refusal; the replicate chooser; support; and `run_tree` end to end on sketches written by the test,
through the `pairs=` and `nj=` hooks."""
import json
import random
import types

import numpy as np
import pytest

import sketch_cases as KC
import sketch_ref as SR
import tree_cases as TC
import tree_ref as R
from test_sketch_rules import EST, write_folder
from varkoder_amd import sketch, tree
from varkoder_amd.cli import parse_args


# ------------------------------------------------------------------ the rule --

def same_record(a, b):
    return a[0] == b[0] and list(a[1]) == list(b[1]) and np.asarray(a[2], dtype=np.float64).tobytes() == np.asarray(b[2], dtype=np.float64).tobytes()


def test_the_two_statements_agree_bit_for_bit():
    mats = [TC.additive(n, n)[0] for n in (3, 4, 5, 8, 17, 40)] + [TC.noisy(n, 50 + n) for n in (6, 23, 70)]
    mats += [TC.arbitrary(n, 60 + n) for n in (7, 31)] + [TC.ones(6), TC.three_identical()] + [TC.invalid(k) for k in TC.INVALID]
    for D in mats:
        assert same_record(R.nj_loop(D), R.nj_np(D)), len(D)
    D = TC.noisy(300, 9)     # a row sum crosses the partial stride
    act = np.ones(300, dtype=bool)
    assert [R.row_sum_loop(D, i, act) for i in (0, 7, 299)] == [float(x) for x in R.row_sums_np(D, np.eye(300, dtype=bool))[[0, 7, 299]]]
    # a partial sum is not the plain sum: the rule, not the arithmetic, fixes the bits
    assert any(R.row_sum_loop(D, i, act) != float(np.sum(D[i])) for i in range(300))


@pytest.mark.parametrize("n", [3, 4, 5, 8, 17, 40, 70])
def test_additive_trees_come_back(n):
    D, edges = TC.additive(n, 1000 + n)
    status, nodes, lengths = R.nj_np(D)
    assert status == 0
    want = TC.tree_splits(n, edges)
    got = R.splits(n, nodes)
    assert len(got) == n - 3 and set(got) == set(want)
    top, kids = R.children(n, nodes)
    leaf, inner = {}, {}
    for t in range(n - 3):
        for child, at in kids[n + t]:
            (leaf if child < n else inner)[child] = lengths[at]
    for child, at in top:
        (leaf if child < n else inner)[child] = lengths[at]
    for x, w in TC.leaf_edges(n, edges).items():
        assert leaf[x] == pytest.approx(w, abs=1e-12)
    # the n - 3 inner edges are the branches above the n - 3 step nodes, each under the split it carries
    for t, sp in enumerate(got):
        assert inner[n + t] == pytest.approx(want[sp], abs=1e-12)
    assert tree.splits(n, nodes) == got and tree.children(n, nodes) == (top, kids)


def test_ties_join_in_the_order_the_rule_says():
    for n in (4, 5, 9):
        _, nodes, _ = R.nj_np(TC.ones(n))
        assert nodes[:2 * (n - 3)].tolist() == [x for t in range(n - 3) for x in (0, t + 1)]   # (0,1), (0,2), (0,3) ..
    D = TC.three_identical()
    _, nodes, lengths = R.nj_np(D)
    joined = [(int(nodes[2 * t]), int(nodes[2 * t + 1])) for t in range(4)]
    assert (1, 3) in joined and joined.index((1, 3)) < min(joined.index(p) for p in joined if 4 in p)   # 1 with 3 first, 4 after
    t = joined.index((1, 3))
    assert lengths[2 * t] == 0.0 and lengths[2 * t + 1] == 0.0
    assert same_record(R.nj_loop(D), R.nj_np(D))


def test_newick_round_trip_with_awkward_names():
    names = ["plain", "with space", "under_score", "it's", "(paren)", "a:b,c;d", "", "x.y-z+1"]
    n = len(names)
    D, _ = TC.additive(n, 77)
    _, nodes, lengths = R.nj_np(D)
    labels = {t: str(10 * t) for t in range(n - 3)}
    text = tree.newick(names, nodes, lengths, labels)
    assert text == R.newick(names, nodes, lengths, labels) and text.endswith(");\n")
    assert tree.quote("x.y-z+1") == "x.y-z+1" and tree.quote("it's") == "'it''s'" and tree.quote("under_score") == "'under_score'"
    name, length, kids = R.read_newick(text.strip())
    assert length is None and name == "" and len(kids) == 3      # unrooted: a trifurcation at the top
    seen_names, seen_lengths, seen_labels = [], [], []

    def walk(node):
        nm, ln, ks = node
        if ks:
            seen_labels.append(nm)
            for k in ks:
                walk(k)
        else:
            seen_names.append(nm)
        if ln is not None:
            seen_lengths.append(ln)
    walk((name, length, kids))
    assert sorted(seen_names) == sorted(names)
    assert sorted(seen_lengths) == sorted(float(x) for x in lengths)        # repr precision: every length exactly
    assert sorted(x for x in seen_labels if x) == sorted(labels.values())


def test_no_negative_branches_keeps_the_path_length():
    D = TC.arbitrary(12, 4)
    _, nodes, lengths = R.nj_np(D)
    assert (lengths[:-3] < 0).any()
    fixed = tree.no_negative(12, lengths)
    assert fixed == R.no_negative(12, lengths) and fixed[-3:] == [float(x) for x in lengths[-3:]]
    changed = 0
    for t in range(9):
        a, b = lengths[2 * t], lengths[2 * t + 1]
        fa, fb = fixed[2 * t], fixed[2 * t + 1]
        assert fa + fb == pytest.approx(a + b, abs=1e-15)
        if a < 0 or b < 0:
            changed += 1
            assert 0.0 in (fa, fb)
            if a + b >= 0:
                assert fa >= 0 and fb >= 0
        else:
            assert (fa, fb) == (a, b)
    assert changed


# ------------------------------------------------------------------ the distances --

def test_vectorised_distances_equal_the_scalar_ones():
    s = 64
    shared = np.array([[0, 0, 1, 17, 63, 64, 5, 64], [0, 0, 1, 17, 63, 64, 5, 1]])
    seen = np.array([[0, 1, 1, 64, 64, 64, 9, 64], [0, 64, 2, 33, 63, 64, 64, 64]])
    jac = sketch.jaccard_np(shared, seen)
    mash = sketch.mash_distance_np(shared, seen, 21)
    for idx in np.ndindex(shared.shape):
        j = sketch.jaccard(int(shared[idx]), int(seen[idx]))
        m = sketch.mash_distance(j, 21)
        assert (np.isnan(jac[idx]) and j is None) or jac[idx] == j
        assert (np.isnan(mash[idx]) and m is None) or (mash[idx] == m and np.signbit(mash[idx]) == np.signbit(m))
    assert np.isnan(jac[0, 0]) and mash[0, 1] == 1.0 and mash[0, 5] == 0.0      # J undefined, J = 0, J = 1
    # the corrected distance: samples with and without estimates, eta of 0, x below and above 1
    a = [1000, 2500, 10, 64, 7]
    g = [9000.0, 26000, None, 500.0, 3.0]
    eta = [0.93, 1.0, 0.5, 0.0, 0.01]
    rng = np.random.default_rng(3)
    n = len(a)
    for k, every in ((21, 1), (31, 4)):
        seen = rng.integers(0, s + 1, (3, n, n))
        shared = (seen * rng.random((3, n, n))).astype(np.int64)
        shared[0], seen[0] = s, s            # J = 1 everywhere
        shared[1, 0], seen[1, 1] = 0, 0      # J = 0 in a row, nothing seen in another
        got = sketch.corrected_distance_np(shared, seen, k, every, a, g, eta)
        cases = {"none": 0, "one": 0, "zero": 0, "between": 0}
        for idx in np.ndindex(got.shape):
            r, i, j = idx
            want = sketch.corrected_distance_eta(sketch.jaccard(int(shared[idx]), int(seen[idx])), k, every, a[i], g[i], eta[i],
                                                 a[j], g[j], eta[j])
            if want is None:
                assert np.isnan(got[idx])
                cases["none"] += 1
            else:
                assert got[idx] == want and np.signbit(got[idx]) == np.signbit(want), idx
                cases["one" if want == 1.0 else "zero" if want == 0.0 else "between"] += 1
        assert all(cases.values()), cases    # J = 0 (D = 1), x >= 1 (D = 0), undefined, and the open interval


def test_jukes_cantor():
    d = np.array([[0.0, 0.1, 0.3], [0.1, 0.0, 0.7499], [0.3, 0.7499, 0.0]])
    got = tree.jukes_cantor(d)
    import math
    for idx in np.ndindex(d.shape):
        assert got[idx] == (0.0 if d[idx] == 0 else -0.75 * math.log(1.0 - 4.0 * d[idx] / 3.0))
    assert not np.signbit(got[0, 0]) and got[0, 1] > d[0, 1]
    assert np.isnan(tree.jukes_cantor(np.array([[0.0, 0.75], [0.75, 0.0]]))[0, 1])
    assert np.isnan(tree.jukes_cantor(np.array([[0.0, np.nan], [1.0, 0.0]]))).sum() == 2


# ------------------------------------------------------------------ replicates and support --

def test_the_replicate_chooser():
    seen = set()
    for seed in (0, 1, 2 ** 64 - 1):
        for r in range(40):
            keep = tree.kept_blocks(seed, r)
            assert keep == R.kept_blocks(seed, r) == tree.kept_blocks(seed, r)
            assert len(keep) == 32 == len(set(keep)) and keep == sorted(keep) and 0 <= keep[0] and keep[-1] < 64
            seen.add(tuple(keep))
    assert len(seen) == 120                                   # another replicate, another choice
    assert tree.kept_blocks(1, 0) == [2, 6, 7, 10, 12, 13, 14, 16, 18, 19, 22, 23, 24, 28, 31, 34, 37, 39, 40, 43, 44, 45, 46, 47, 50, 52, 56, 57, 58, 59, 61, 63]   # stable for a seed
    used = np.zeros(64)
    for r in range(400):
        used[tree.kept_blocks(7, r)] += 1
    assert used.min() > 150 and used.max() < 250              # every block kept about half the time
    assert tree.mix(12345) == SR.mix(12345) == R.mix(12345)


def test_support_counts():
    n = 9
    D, _ = TC.additive(n, 5)
    _, nodes, _ = R.nj_np(D)
    other = R.nj_np(TC.additive(n, 6)[0])[1]
    assert R.support(n, nodes, [nodes] * 7) == [7] * (n - 3)
    mixed = R.support(n, nodes, [nodes, other, other])
    absent = [sp not in set(R.splits(n, other)) for sp in R.splits(n, nodes)]
    assert any(absent) and mixed == [1 if a else 3 for a in absent]
    assert tree.percent(7, 7) == 100 and tree.percent(0, 7) == 0 and tree.percent(1, 3) == 33 and tree.percent(1, 2) == 50
    assert tree.percent(2, 3) == 67 and tree.percent(1, 8) == 13


# ------------------------------------------------------------------ the command --

def ref_pairs(q, ql, r, rl, s, blocks=False):
    n = len(q)
    if blocks:
        out = np.zeros((2, n, n, 64), dtype=np.uint32)
        for i in range(n):
            for j in range(n):
                out[0, i, j], out[1, i, j] = R.pair_blocks_loop(q[i, :int(ql[i])], r[j, :int(rl[j])], s)
        return out[0], out[1]
    out = np.zeros((2, n, n), dtype=np.uint32)
    for i in range(n):
        for j in range(n):
            out[:, i, j] = SR.pair_loop(q[i, :int(ql[i])], r[j, :int(rl[j])], s)
    return out[0], out[1]


def ref_nj(D):
    return R.nj_batch(D)


def args_of(inp, out, matrix_from=None, distance="corrected", jc=False, replicates=0, seed=1, nonneg=False, overwrite=False):
    return types.SimpleNamespace(input=None if inp is None else str(inp), outdir=str(out),
                                 matrix_from=None if matrix_from is None else str(matrix_from), distance=distance, jukes_cantor=jc,
                                 replicates=replicates, seed=seed, no_negative_branches=nonneg, overwrite=overwrite)


def family(seed=3, size=256, n=6):
    """Sketches of n relatives: sample i shares a falling part of a common pool with the first."""
    rng = random.Random(seed)
    pool = KC.spread(rng, 6 * size)
    est = {"kmer_coverage": 30.0, "genome_kmers": float(size + 3)}
    out = {}
    for i in range(n):
        own = pool[size * (i + 1):size * (i + 1) + 40 * i + (i % 2) * 9]
        out["s%d" % i] = (sorted(pool[:size - len(own)] + own), est)
    return out


def test_run_tree_end_to_end_through_the_hooks(tmp_path):
    samples = family()
    write_folder(tmp_path / "D", samples, size=256)
    names = sorted(samples)
    out = tree.run_tree(args_of(tmp_path / "D", tmp_path / "OUT", replicates=12, seed=5), pairs=ref_pairs, nj=ref_nj)
    back = json.loads((tmp_path / "OUT" / "tree.json").read_text())
    assert back == out and back["names"] == names and back["distance"] == "corrected" and back["transform"] is None
    assert back["replicates"] == {"asked": 12, "used": 12, "dropped": 0} and back["seed"] == 5
    n = len(names)
    # the same by hand, from the reference functions
    hashes = [np.array(samples[x][0], dtype=np.uint64) for x in names]
    sh = np.zeros((n, n, 64), dtype=np.int64)
    se = np.zeros((n, n, 64), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            sh[i, j], se[i, j] = R.pair_blocks_loop(hashes[i], hashes[j], 256)

    def dist(shared, seen):
        d = np.zeros((n, n))
        for i in range(n):
            for j in range(n):
                if i != j:
                    eta, g = sketch.sample_eta(samples[names[i]][1], 1)
                    d[i, j] = sketch.corrected_distance_eta(sketch.jaccard(int(shared[i, j]), int(seen[i, j])), 21, 1,
                                                            len(hashes[i]) + 3, g, eta, len(hashes[j]) + 3, g, eta)
        return d
    main = R.nj_np(dist(sh.sum(-1), se.sum(-1)))
    assert main[0] == 0 and back["nodes"] == main[1].tolist() and back["lengths"] == main[2].tolist()
    reps = [R.nj_np(dist(sh[..., R.kept_blocks(5, r)].sum(-1), se[..., R.kept_blocks(5, r)].sum(-1)))[1] for r in range(12)]
    counts = R.support(n, main[1], reps)
    assert [sp["support"] for sp in back["splits"]] == counts
    assert [sp["leaves"] for sp in back["splits"]] == [sorted(sp) for sp in R.splits(n, main[1])]
    labels = {t: str(tree.percent(c, 12)) for t, c in enumerate(counts)}
    assert (tmp_path / "OUT" / "tree.nwk").read_text() == R.newick(names, main[1], main[2], labels)
    # mash, Jukes-Cantor, no replicates, no negative branches
    out = tree.run_tree(args_of(tmp_path / "D", tmp_path / "OUT2", distance="mash", jc=True, nonneg=True), pairs=ref_pairs, nj=ref_nj)
    assert out["distance"] == "mash" and out["transform"] == "jukes-cantor" and out["replicates"]["used"] == 0
    assert all(sp["support"] is None for sp in out["splits"])
    d = tree.jukes_cantor(sketch.mash_distance_np(sh.sum(-1), se.sum(-1), 21) * (1 - np.eye(n)))
    ref = R.nj_np(d)
    assert out["nodes"] == ref[1].tolist() and out["lengths"] == ref[2].tolist()
    assert (tmp_path / "OUT2" / "tree.nwk").read_text() == R.newick(names, ref[1], R.no_negative(n, ref[2]))


def test_matrix_from(tmp_path):
    n = 7
    D = TC.noisy(n, 8)
    names = ["m%d" % i for i in range(n)]

    def folder(name, mat, file="corrected_distance.npy", rows=names, cols=names):
        f = tmp_path / name
        f.mkdir()
        np.save(f / file, mat)
        (f / "distances_rows.txt").write_text("".join(x + "\n" for x in rows))
        (f / "distances_cols.txt").write_text("".join(x + "\n" for x in cols))
        return f
    out = tree.run_tree(args_of(None, tmp_path / "O1", matrix_from=folder("M1", D)), pairs=ref_pairs, nj=ref_nj)
    ref = R.nj_np(D)
    assert out["distance"] == "matrix" and out["nodes"] == ref[1].tolist() and out["lengths"] == ref[2].tolist()
    assert (tmp_path / "O1" / "tree.nwk").read_text() == R.newick(names, ref[1], ref[2])
    # compare --matrix: uint64
    U = (D * 1000).astype(np.uint64)
    U = np.maximum(U, U.T)
    out = tree.run_tree(args_of(None, tmp_path / "O2", matrix_from=folder("M2", U, "distances.npy")), pairs=ref_pairs, nj=ref_nj)
    assert out["nodes"] == R.nj_np(U.astype(np.float64))[1].tolist()
    big = U.copy()
    big[1, 2] = big[2, 1] = 2 ** 53 + 1
    with pytest.raises(Exception, match="2\\^53.*m1 and m2"):
        tree.run_tree(args_of(None, tmp_path / "O3", matrix_from=folder("M3", big, "distances.npy")), pairs=ref_pairs, nj=ref_nj)
    with pytest.raises(Exception, match="not its columns"):
        tree.run_tree(args_of(None, tmp_path / "O4", matrix_from=folder("M4", D, cols=names[::-1])), pairs=ref_pairs, nj=ref_nj)
    with pytest.raises(Exception, match="not a square"):
        tree.run_tree(args_of(None, tmp_path / "O5", matrix_from=folder("M5", D[:, :5])), pairs=ref_pairs, nj=ref_nj)
    nan = D.copy()
    nan[0, 3] = nan[3, 0] = np.nan
    with pytest.raises(Exception, match="m0 and m3"):
        tree.run_tree(args_of(None, tmp_path / "O6", matrix_from=folder("M6", nan)), pairs=ref_pairs, nj=ref_nj)
    with pytest.raises(Exception, match="not symmetric: m3 and m4"):
        tree.run_tree(args_of(None, tmp_path / "O7", matrix_from=folder("M7", TC.invalid("asymmetric", n))), pairs=ref_pairs, nj=ref_nj)
    (tmp_path / "M8").mkdir()
    with pytest.raises(Exception, match="no corrected_distance.npy"):
        tree.run_tree(args_of(None, tmp_path / "O8", matrix_from=tmp_path / "M8"), pairs=ref_pairs, nj=ref_nj)
    with pytest.raises(Exception, match="--replicates"):
        tree.run_tree(args_of(None, tmp_path / "O9", matrix_from=tmp_path / "M1", replicates=3), pairs=ref_pairs, nj=ref_nj)
    with pytest.raises(Exception, match="3 to"):
        tree.run_tree(args_of(None, tmp_path / "O10", matrix_from=folder("M10", D[:2, :2], rows=names[:2], cols=names[:2])),
                      pairs=ref_pairs, nj=ref_nj)


def test_refusals(tmp_path, monkeypatch):
    samples = family()
    write_folder(tmp_path / "D", samples, size=256)
    (tmp_path / "OUT").mkdir()
    with pytest.raises(Exception, match="exists"):
        tree.run_tree(args_of(tmp_path / "D", tmp_path / "OUT"), pairs=ref_pairs, nj=ref_nj)
    tree.run_tree(args_of(tmp_path / "D", tmp_path / "OUT", overwrite=True), pairs=ref_pairs, nj=ref_nj)
    with pytest.raises(Exception, match="does not exist"):
        tree.run_tree(args_of(tmp_path / "nowhere", tmp_path / "O2"), pairs=ref_pairs, nj=ref_nj)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(Exception, match="one GPU"):
        tree.run_tree(args_of(tmp_path / "D", tmp_path / "O3"), pairs=ref_pairs, nj=ref_nj)
    monkeypatch.delenv("WORLD_SIZE")
    # check_comparable applies as in `distance`
    write_folder(tmp_path / "X", samples, size=256, s1={"k": 25})
    with pytest.raises(Exception, match="do not compare"):
        tree.run_tree(args_of(tmp_path / "X", tmp_path / "O4"), pairs=ref_pairs, nj=ref_nj)
    # an undefined distance in the main matrix: a sample without estimates (corrected), an empty pair of sketches (both)
    noest = dict(samples, s2=(samples["s2"][0], None))
    write_folder(tmp_path / "N", noest, size=256)
    with pytest.raises(Exception, match="no corrected distance between s0 and s2"):
        tree.run_tree(args_of(tmp_path / "N", tmp_path / "O5"), pairs=ref_pairs, nj=ref_nj)
    tree.run_tree(args_of(tmp_path / "N", tmp_path / "O5", distance="mash"), pairs=ref_pairs, nj=ref_nj)   # (mash needs none)
    empty = dict(samples, s4=([], EST))
    write_folder(tmp_path / "E", empty, size=256)
    with pytest.raises(Exception, match="no mash distance between s4 and s4"):
        tree.run_tree(args_of(tmp_path / "E", tmp_path / "O6", distance="mash"), pairs=ref_pairs, nj=ref_nj)
    # Jukes-Cantor: disjoint sketches are at Mash distance 1
    rng = random.Random(1)
    pool = KC.spread(rng, 1024)
    far = {"a": (pool[0:256], EST), "b": (pool[0:256:2] + pool[256:384], EST), "c": (pool[512:768], EST)}
    write_folder(tmp_path / "F", {k: (sorted(v[0]), v[1]) for k, v in far.items()}, size=256)
    with pytest.raises(Exception, match="--jukes-cantor: the distance between a and c is 0.75 or more"):
        tree.run_tree(args_of(tmp_path / "F", tmp_path / "O7", distance="mash", jc=True), pairs=ref_pairs, nj=ref_nj)
    # two samples are no tree
    write_folder(tmp_path / "T", {k: samples[k] for k in ("s0", "s1")}, size=256)
    with pytest.raises(Exception, match="3 to"):
        tree.run_tree(args_of(tmp_path / "T", tmp_path / "O8"), pairs=ref_pairs, nj=ref_nj)
    # the device's own refusal reaches the user
    with pytest.raises(Exception, match="refused matrix 0"):
        tree.run_tree(args_of(tmp_path / "D", tmp_path / "O9"), pairs=ref_pairs,
                      nj=lambda D: (np.ones(len(D), dtype=np.uint32),) + R.nj_batch(D)[1:])


def test_replicates_with_undefined_distances_are_dropped_and_counted(tmp_path):
    """tiny sketches: a replicate that keeps no seen value of some pair has no distance there"""
    rng = random.Random(5)
    pool = KC.spread(rng, 64)
    tiny = {"t%d" % i: (sorted(rng.sample(pool, 3)), EST) for i in range(4)}
    write_folder(tmp_path / "D", tiny, size=64)
    names = sorted(tiny)
    sh = np.zeros((4, 4, 64), dtype=np.int64)
    se = np.zeros((4, 4, 64), dtype=np.int64)
    for i in range(4):
        for j in range(4):
            sh[i, j], se[i, j] = R.pair_blocks_loop(tiny[names[i]][0], tiny[names[j]][0], 64)
    asked = 40
    dropped = sum(1 for r in range(asked) if (se[..., R.kept_blocks(2, r)].sum(-1) == 0).any())
    assert 0 < dropped < asked
    if 2 * dropped > asked:
        with pytest.raises(Exception, match="more than half"):
            tree.run_tree(args_of(tmp_path / "D", tmp_path / "OUT", distance="mash", replicates=asked, seed=2), pairs=ref_pairs, nj=ref_nj)
    else:
        out = tree.run_tree(args_of(tmp_path / "D", tmp_path / "OUT", distance="mash", replicates=asked, seed=2), pairs=ref_pairs, nj=ref_nj)
        assert out["replicates"] == {"asked": asked, "used": asked - dropped, "dropped": dropped}
    # and with one-value sketches nearly every replicate is dropped: refused
    one = {"u%d" % i: ([pool[i]], EST) for i in range(4)}
    write_folder(tmp_path / "U", one, size=64)
    with pytest.raises(Exception, match="more than half"):
        tree.run_tree(args_of(tmp_path / "U", tmp_path / "OUT3", distance="mash", replicates=20, seed=2), pairs=ref_pairs, nj=ref_nj)


def test_the_command_line():
    a = parse_args(["tree", "S", "O", "--replicates", "100", "--seed", "9", "--distance", "mash", "--jukes-cantor", "-x"])
    assert (a.input, a.outdir, a.matrix_from, a.replicates, a.seed, a.distance, a.jukes_cantor, a.overwrite, a.no_negative_branches) == \
        ("S", "O", None, 100, 9, "mash", True, True, False)
    a = parse_args(["tree", "--matrix-from", "M", "O", "--no-negative-branches"])
    assert (a.input, a.outdir, a.matrix_from, a.replicates, a.no_negative_branches) == ("M", "O", "M", 0, True)
    for bad in (["tree", "S"], ["tree", "--matrix-from", "M", "S", "O"], ["tree", "--matrix-from", "M", "O", "--replicates", "3"],
                ["tree", "S", "O", "--replicates", "4096"], ["tree", "S", "O", "--replicates", "-1"],
                ["tree", "--matrix-from", "M", "O", "--jukes-cantor"]):
        with pytest.raises(SystemExit):
            parse_args(bad)
