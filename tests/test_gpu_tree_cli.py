"""`tree` end to end.  `image --from-clean --kmer-spectrum D --spectrum-sketch 64` on seven tiny synthetic samples -- a
genome, five relatives at rising divergence, a stranger -- then `tree D OUT --replicates 20`: tree.nwk and tree.json are what
tests/tree_ref.py and the scalar functions of varkoder_amd/sketch.py give for the same files (per-block counts by the loop,
every distance by the scalar function, the joins by the rule's NumPy statement, the blocks by the chooser written out in
tree_ref).  Then `distance D M --matrix` and `tree --matrix-from M OUT2`: the tree of that matrix by the rule."""
import gzip
import json

import numpy as np
import pytest

import tree_ref as R
from screen_cases import fq
from test_gpu_write_splits import run
from varkoder_amd import cli, sketch, tree

pytestmark = pytest.mark.gpu

COMMON = ["-R", "7", "-m", "5K", "-M", "20K", "-k", "7"]
SIZE, REPS, SEED = 64, 20, 11


def clean_texts():
    rng = np.random.default_rng(21)
    g = rng.integers(0, 4, 8000, dtype=np.uint8)

    def mutated(d):
        out = g.copy()
        sub = rng.random(len(g)) < d
        out[sub] = (out[sub] + rng.integers(1, 4, int(sub.sum()), dtype=np.uint8)) & 3
        return out

    def reads(genome, n):
        at = rng.integers(0, len(genome) - 100 + 1, n)
        r = genome[at[:, None] + np.arange(100)[None, :]]
        return fq([x.tobytes() for x in np.frombuffer(b"ACGT", dtype=np.uint8)[r]])
    texts = {"g_0": reads(g, 1600)}
    for i, d in enumerate((0.002, 0.005, 0.01, 0.02, 0.04)):
        texts["rel_%d" % (i + 1)] = reads(mutated(d), 1600)
    texts["stranger"] = reads(rng.integers(0, 4, 8000, dtype=np.uint8), 1600)
    return texts


def by_the_reference(folder, names, which):
    """(main record, support counts, used) from the folder's files through the reference functions alone."""
    reports = [json.loads((folder / f"{s}.spectrum.json").read_text()) for s in names]
    hashes = [np.load(folder / f"{s}.sketch.npy") for s in names]
    n = len(names)
    sh, se = np.zeros((n, n, 64), dtype=np.int64), np.zeros((n, n, 64), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            sh[i, j], se[i, j] = R.pair_blocks_loop(hashes[i], hashes[j], SIZE)

    def dist(shared, seen):
        d = np.zeros((n, n))
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                jac = sketch.jaccard(int(shared[i, j]), int(seen[i, j]))
                a, b = reports[i], reports[j]
                eta1, g1 = sketch.sample_eta(a["estimates"], a["sketch"]["min_count"])
                eta2, g2 = sketch.sample_eta(b["estimates"], b["sketch"]["min_count"])
                v = sketch.mash_distance(jac, a["k"]) if which == "mash" else sketch.corrected_distance_eta(
                    jac, a["k"], a["every"], a["sketch"]["eligible"], g1, eta1, b["sketch"]["eligible"], g2, eta2)
                d[i, j] = np.nan if v is None else v
        return d
    main = R.nj_np(dist(sh.sum(-1), se.sum(-1)))
    reps = []
    for r in range(REPS):
        keep = R.kept_blocks(SEED, r)
        d = dist(sh[..., keep].sum(-1), se[..., keep].sum(-1))
        if not np.isnan(d).any() and not (se[..., keep].sum(-1) == 0).any():
            reps.append(R.nj_np(d)[1])
    return main, R.support(n, main[1], reps), len(reps)


def test_tree_of_seven_sketched_samples_and_of_their_matrix(tmp_path):
    texts = clean_texts()
    (tmp_path / "int" / "clean_reads").mkdir(parents=True)
    for s, t in texts.items():
        (tmp_path / "int" / "clean_reads" / f"{s}.fq.gz").write_bytes(gzip.compress(t, compresslevel=1))
    run(["--from-clean", "int", "-o", "img", "-f", "s.csv", "--kmer-spectrum", "D", "--spectrum-sketch", str(SIZE)] + COMMON, tmp_path)
    names = sorted(texts)
    assert len(names) == 7
    cli.main(["tree", str(tmp_path / "D"), str(tmp_path / "OUT"), "--replicates", str(REPS), "--seed", str(SEED)])
    got = json.loads((tmp_path / "OUT" / "tree.json").read_text())
    main, counts, used = by_the_reference(tmp_path / "D", names, "corrected")
    assert main[0] == 0 and got["names"] == names and got["distance"] == "corrected" and got["seed"] == SEED
    assert got["nodes"] == main[1].tolist() and got["lengths"] == main[2].tolist()      # bit for bit: json keeps repr
    assert got["replicates"] == {"asked": REPS, "used": used, "dropped": REPS - used} and 2 * used >= REPS
    assert [sp["support"] for sp in got["splits"]] == counts
    assert [sp["leaves"] for sp in got["splits"]] == [sorted(sp) for sp in R.splits(7, main[1])]
    labels = {t: str(tree.percent(c, used)) for t, c in enumerate(counts)}
    assert (tmp_path / "OUT" / "tree.nwk").read_text() == R.newick(names, main[1], main[2], labels)
    # the stranger hangs off the longest branch
    top, kids = R.children(7, main[1])
    branch = {c: main[2][at] for t in kids for c, at in kids[t]} | {c: main[2][at] for c, at in top}
    assert max((v, c) for c, v in branch.items() if c < 7)[1] == names.index("stranger")
    # mash, no replicates: another engine call path (vk_sketch_pairs_device)
    cli.main(["tree", str(tmp_path / "D"), str(tmp_path / "OUTM"), "--distance", "mash", "--no-negative-branches"])
    gm = json.loads((tmp_path / "OUTM" / "tree.json").read_text())
    mm = by_the_reference(tmp_path / "D", names, "mash")[0]
    assert gm["nodes"] == mm[1].tolist() and gm["lengths"] == mm[2].tolist() and gm["replicates"]["used"] == 0
    assert (tmp_path / "OUTM" / "tree.nwk").read_text() == R.newick(names, mm[1], R.no_negative(7, mm[2]))
    # the matrix that `distance --matrix` writes, joined as it is
    cli.main(["distance", str(tmp_path / "D"), str(tmp_path / "M"), "--matrix"])
    cli.main(["tree", "--matrix-from", str(tmp_path / "M"), str(tmp_path / "OUT2")])
    g2 = json.loads((tmp_path / "OUT2" / "tree.json").read_text())
    m = np.load(tmp_path / "M" / "corrected_distance.npy")
    np.fill_diagonal(m, 0.0)
    ref = R.nj_np(m)
    assert g2["distance"] == "matrix" and g2["names"] == names and g2["nodes"] == ref[1].tolist() and g2["lengths"] == ref[2].tolist()
    assert g2["nodes"] == got["nodes"] and g2["lengths"] == got["lengths"]   # the same distances either way
    assert (tmp_path / "OUT2" / "tree.nwk").read_text() == R.newick(names, ref[1], ref[2])
    with pytest.raises(Exception, match="exists"):
        cli.main(["tree", str(tmp_path / "D"), str(tmp_path / "OUT")])
