"""`tree`: a neighbour-joining tree of the samples of a folder of sketches, with jackknife support, or of a distance matrix
that `distance --matrix` or `compare --matrix` wrote.  Neither the reference nor any other command here builds a tree;
the rule is this project's ("`tree`: the rule").

From sketches: one call compares every pair (ImageEngine.sketch_pairs, or with --replicates ImageEngine.sketch_pair_blocks,
which splits a pair's two counts by the block h & 63 of each sketch value); the distances -- `corrected_distance` or
`mash_distance` of every pair, sketch.py's vectorised forms -- are computed on the host from the integers.  Replicate r keeps
32 of the 64 blocks (kept_blocks: splitmix64 steps driving a Fisher-Yates shuffle, from --seed and r); its shared and seen
are the sums of the kept blocks' counts and its distances come from those, every sample's eligible, eta and G unchanged.
The main matrix and every kept replicate then go through ONE call of ImageEngine.nj (vk_tree_nj_device, csrc/vk_tree.h);
there is no CPU path for the joining.  A split's support is the number of replicate trees that contain it.

What the support measures: the blocks partition the sketch's hash space, so this delete-half jackknife resamples the
SKETCH -- it says how far the tree depends on which k-mers the sketch happened to sample.  It does not resample reads or
loci: a well-supported split can still be wrong when the distances are biased, and support rises with the sketch size.

Outputs in OUT: tree.nwk (Newick, unrooted, a trifurcation at the top) and tree.json (names, distance, the join record as
the device wrote it, replicates asked for and used, seed, every split with its support count).
"""
import json
import math
import re
from pathlib import Path

import numpy as np

from . import sketch
from .image import eprint

BLOCKS, KEPT = 64, 32
MASK = (1 << 64) - 1
GOLDEN, C1, C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MIN_LEAVES, MAX_LEAVES, MAX_TREES, MAX_ENTRY = 3, 16384, 4096, 1e100
MAX_EXACT = 1 << 53


# ----------------------------------------------------------------------------------------------- the replicates --

def mix(z):
    """splitmix64's finaliser."""
    z = ((z ^ (z >> 30)) * C1) & MASK
    z = ((z ^ (z >> 27)) * C2) & MASK
    return z ^ (z >> 31)


def kept_blocks(seed, r):
    """The 32 blocks that replicate r keeps, ascending.  The generator is written out here, so that a seed means the same
    replicates with every NumPy: state = mix(seed + GOLDEN) ^ r; an output is mix(state += GOLDEN); a Fisher-Yates shuffle
    of 0 .. 63 from the top down takes one output per swap (j = output mod (i + 1): the bias is below 2^-57); the first
    32 of the shuffled list are kept."""
    state = mix((seed + GOLDEN) & MASK) ^ (r & MASK)
    order = list(range(BLOCKS))
    for i in range(BLOCKS - 1, 0, -1):
        state = (state + GOLDEN) & MASK
        j = mix(state) % (i + 1)
        order[i], order[j] = order[j], order[i]
    return sorted(order[:KEPT])


# ------------------------------------------------------------------------------------------- records and Newick --

def record_len(n):
    return 2 * (n - 3) + 3


def children(n, nodes):
    """(top, kids) of a join record: kids[n + t] = the two (child, index of the branch's length) of step t's node, top
    the three of the trifurcation; leaves are 0 .. n - 1."""
    slot = list(range(n))
    kids = {}
    for t in range(n - 3):
        i, j = int(nodes[2 * t]), int(nodes[2 * t + 1])
        kids[n + t] = ((slot[i], 2 * t), (slot[j], 2 * t + 1))
        slot[i] = n + t
    base = 2 * (n - 3)
    return [(slot[int(nodes[base + x])], base + x) for x in range(3)], kids


def splits(n, nodes):
    """The bipartition under every step's node, normalised to the side without leaf 0 (a frozenset of leaves), in step
    order: the n - 3 inner edges of the unrooted tree."""
    _, kids = children(n, nodes)
    under, out, everyone = {}, [], frozenset(range(n))
    for t in range(n - 3):
        leaves = frozenset()
        for child, _ in kids[n + t]:
            leaves |= under[child] if child >= n else frozenset([child])
        under[n + t] = leaves
        out.append(everyone - leaves if 0 in leaves else leaves)
    return out


def no_negative(n, lengths):
    """Kuhner and Felsenstein (1994): of a joined pair a negative length becomes 0 and its sibling takes the difference,
    so the path through the pair keeps its length.  The closing three have no single sibling and stay as computed."""
    out = [float(x) for x in lengths]
    for t in range(n - 3):
        li, lj = out[2 * t], out[2 * t + 1]
        if li < 0.0:
            out[2 * t], out[2 * t + 1] = 0.0, lj + li
        elif lj < 0.0:
            out[2 * t], out[2 * t + 1] = li + lj, 0.0
    return out


PLAIN = re.compile(r"[A-Za-z0-9.+-]+\Z")


def quote(name):
    """A Newick label: as it is when it holds only letters, digits, '.', '+' and '-'; else in single quotes, a quote
    doubled (an unquoted underscore would be read as a blank, so a name with one is quoted)."""
    return name if PLAIN.match(name) else "'" + name.replace("'", "''") + "'"


def newick(names, nodes, lengths, labels=None):
    """tree.nwk's text; labels: {step: text} for the inner nodes.  Lengths with repr precision."""
    n = len(names)
    top, kids = children(n, nodes)
    labels = labels or {}
    done = {}
    for node in sorted(kids):   # (children before parents: no recursion, whatever the depth)
        parts = []
        for child, at in kids[node]:
            body = quote(names[child]) if child < n else done.pop(child)
            parts.append(body + ":" + repr(float(lengths[at])))
        done[node] = "(" + ",".join(parts) + ")" + labels.get(node - n, "")
    parts = [(quote(names[c]) if c < n else done.pop(c)) + ":" + repr(float(lengths[at])) for c, at in top]
    return "(" + ",".join(parts) + ");\n"


def percent(count, used):
    """Support as an integer percentage, halves up."""
    return (200 * count + used) // (2 * used)


# ------------------------------------------------------------------------------------------------ the distances --

def first_pair(names, bad):
    i, j = (int(x) for x in np.argwhere(bad)[0])
    return names[i], names[j]


def sample_values(st):
    """(k, every, a, g, eta) of a SketchSet: what corrected_distance_np takes per sample."""
    a, g, eta = [], [], []
    for rep in st.reports:
        e, gg = sketch.sample_eta(rep["estimates"], rep["sketch"]["min_count"])
        a.append(rep["sketch"]["eligible"])
        g.append(gg)
        eta.append(e)
    return st.reports[0]["k"], st.reports[0]["every"], a, g, eta


def distances_of(st, shared, seen, which):
    """The distance matrices of integer counts [..., n, n]: float64, NaN where a distance is undefined, the diagonal 0."""
    k, every, a, g, eta = sample_values(st)
    if which == "mash":
        d = sketch.mash_distance_np(shared, seen, k)
    else:
        d = sketch.corrected_distance_np(shared, seen, k, every, a, g, eta)
    n = d.shape[-1]
    idx = np.arange(n)
    d[..., idx, idx] = np.where(np.isnan(d[..., idx, idx]), np.nan, 0.0)
    return d


def jukes_cantor(d):
    """-0.75 ln(1 - 4 D / 3) of every entry below 0.75; NaN from 0.75 on (and where D is NaN)."""
    with np.errstate(invalid="ignore"):
        ok = d < 0.75
    x = np.where(ok, 1.0 - 4.0 * d / 3.0, 1.0)
    out = -0.75 * sketch._map(math.log, x)
    out = np.where(out > 0.0, out, 0.0)   # (-0.0 at D = 0)
    return np.where(ok, out, np.nan)


def check_matrix(d, names):
    """What vk_tree_nj_device would flag, refused here with the first pair's names."""
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(d) | ~(d >= 0.0) | ~(d <= MAX_ENTRY)
    if bad.any():
        raise Exception("a distance that is not finite, negative or above 1e100: %s and %s" % first_pair(names, bad))
    if (np.diagonal(d) != 0.0).any():
        raise Exception("a sample at a distance from itself: %s" % names[int(np.flatnonzero(np.diagonal(d) != 0.0)[0])])
    bad = d.view(np.uint64) != d.T.view(np.uint64)
    if bad.any():
        raise Exception("a matrix that is not symmetric: %s and %s" % first_pair(names, bad))


def matrix_from(folder):
    """(names, matrix float64, file) of a folder that `distance --matrix` (corrected_distance.npy) or `compare --matrix`
    (distances.npy, uint64) wrote.  The file's diagonal is not read: it is 0 in the matrix that is joined."""
    folder = Path(folder)
    rows, cols = folder / "distances_rows.txt", folder / "distances_cols.txt"
    path = next((p for p in (folder / "corrected_distance.npy", folder / "distances.npy") if p.exists()), None)
    if path is None or not rows.exists() or not cols.exists():
        raise Exception(f"{folder}: no corrected_distance.npy or distances.npy with distances_rows.txt and distances_cols.txt "
                        "(written by `distance --matrix` or `compare --matrix`)")
    names = rows.read_text().splitlines()
    if names != cols.read_text().splitlines():
        raise Exception(f"{folder}: the rows of the matrix are not its columns (a matrix made with --against is no tree's)")
    m = np.load(path)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] != len(names):
        raise Exception(f"{path}: not a square matrix of its {len(names)} names: shape {m.shape}")
    if m.dtype == np.uint64:
        if m.size and int(m.max()) > MAX_EXACT:
            raise Exception("%s: a distance above 2^53 is no exact double: %s and %s" % ((path,) + first_pair(names, m > MAX_EXACT)))
    elif m.dtype != np.float64:
        raise Exception(f"{path}: float64 or uint64 expected, not {m.dtype}")
    m = np.array(m, dtype=np.float64)
    np.fill_diagonal(m, 0.0)   # (not read: a sample is at 0 from itself, and `distance` writes its estimate of that there)
    return names, m, path


# --------------------------------------------------------------------------------------------------- the command --

def refuse_early(args):
    """What can be refused before anything is read or the GPU is touched."""
    from .shard import world_info
    if world_info()[1] > 1:
        raise Exception("tree runs on one GPU: start it without a launcher (WORLD_SIZE > 1 is refused; the joining is not sharded)")
    src = args.matrix_from or args.input
    if not Path(src).exists():
        raise Exception("Input path", src, "does not exist. Please check.")
    if not args.overwrite and Path(args.outdir).exists():
        raise Exception("Output directory exists, use --overwrite if you want to overwrite it.")
    if args.matrix_from and args.replicates:
        raise Exception("--replicates: not with --matrix-from (a matrix carries no sketch to resample)")
    if not 0 <= args.replicates < MAX_TREES:
        raise Exception(f"--replicates: 0 to {MAX_TREES - 1}")


def check_count(names):
    if not MIN_LEAVES <= len(names) <= MAX_LEAVES:
        raise Exception(f"a tree needs {MIN_LEAVES} to {MAX_LEAVES} samples: {len(names)} found")
    if len(set(names)) != len(names):
        raise Exception("two samples of one name")


def engine_calls(pairs, nj):
    """(pairs, nj, close): the hooks, or the engine's calls."""
    if pairs is not None and nj is not None:
        return pairs, nj, lambda: None
    from .engine import ImageEngine
    from .shard import world_info
    eng = ImageEngine(k=7, mapping="cgr", device=world_info()[2])   # (k and mapping are not used)

    def eng_pairs(q, ql, r, rl, s, blocks=False):
        return (eng.sketch_pair_blocks if blocks else eng.sketch_pairs)(q, ql, r, rl, s)
    return pairs or eng_pairs, nj or eng.nj, eng.close


def run_tree(args, pairs=None, nj=None):
    """The `tree` sub-command; returns tree.json's object as written.  Hooks (tests): pairs, a function (q rows, q
    lengths, r rows, r lengths, size, blocks=False) -> (shared, seen), with blocks=True [n, n, 64] each, in place of the
    engine's; nj, a function (float64 [ntrees, n, n]) -> (status, nodes, lengths) in place of ImageEngine.nj."""
    refuse_early(args)
    eprint("Starting tree command.")
    asked = int(args.replicates)
    if args.matrix_from:
        names, main, path = matrix_from(args.matrix_from)
        check_count(names)
        which, source, st = "matrix", str(path), None
    else:
        from .distance import SketchSet, check_comparable
        st = SketchSet(args.input)
        check_comparable([st])
        names, which, source = st.names, args.distance, str(args.input)
        check_count(names)
    pairs, nj, close = engine_calls(pairs, nj)
    try:
        reps = []
        if st is not None:
            eprint(f"Comparing {len(names)} sketches, every pair.")
            if asked:
                shared_b, seen_b = pairs(st.rows, st.lengths, st.rows, st.lengths, st.size, blocks=True)
                shared_b, seen_b = shared_b.astype(np.int64), seen_b.astype(np.int64)
                shared, seen = shared_b.sum(axis=-1), seen_b.sum(axis=-1)
            else:
                shared, seen = pairs(st.rows, st.lengths, st.rows, st.lengths, st.size)
            main = distances_of(st, shared, seen, which)
            if np.isnan(main).any():
                raise Exception("no %s distance between %s and %s (nothing seen, or a sample without estimates)"
                                % ((which,) + first_pair(names, np.isnan(main))))
            if args.jukes_cantor:
                main = jukes_cantor(main)
                if np.isnan(main).any():
                    raise Exception("--jukes-cantor: the distance between %s and %s is 0.75 or more"
                                    % first_pair(names, np.isnan(main)))
            for r in range(asked):
                keep = kept_blocks(args.seed, r)
                d = distances_of(st, shared_b[..., keep].sum(axis=-1), seen_b[..., keep].sum(axis=-1), which)
                if args.jukes_cantor:
                    d = jukes_cantor(d)
                if not np.isnan(d).any():
                    reps.append(d)
            if asked and 2 * (asked - len(reps)) > asked:
                raise Exception(f"{asked - len(reps)} of {asked} replicates hold an undefined distance: more than half; "
                                "the sketches are too small for a delete-half jackknife")
        check_matrix(main, names)
        eprint(f"Joining {1 + len(reps)} matrices of {len(names)} samples.")
        status, nodes, lengths = nj(np.stack([main] + reps))
    finally:
        close()
    if status.any():
        raise Exception(f"vk_tree_nj_device refused matrix {int(np.flatnonzero(status)[0])} (0 is the main one): status "
                        f"{int(status[np.flatnonzero(status)[0]])}")
    n = len(names)
    main_splits = splits(n, nodes[0])
    have = [set(splits(n, nodes[r])) for r in range(1, 1 + len(reps))]
    counts = [sum(1 for h in have if sp in h) for sp in main_splits]
    labels = {t: str(percent(c, len(reps))) for t, c in enumerate(counts)} if reps else None
    shown = no_negative(n, lengths[0]) if args.no_negative_branches else lengths[0]
    out = {"names": list(names), "source": source, "distance": which,
           "transform": "jukes-cantor" if (st is not None and args.jukes_cantor) else None,
           "nodes": [int(x) for x in nodes[0]], "lengths": [float(x) for x in lengths[0]],
           "no_negative_branches": bool(args.no_negative_branches),
           "replicates": {"asked": asked, "used": len(reps), "dropped": asked - len(reps)}, "seed": int(args.seed),
           "splits": [{"step": t, "leaves": sorted(sp), "support": (counts[t] if reps else None)} for t, sp in enumerate(main_splits)]}
    outdir = Path(args.outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    (outdir / "tree.nwk").write_text(newick(names, nodes[0], shown, labels))
    (outdir / "tree.json").write_text(json.dumps(out, indent=1) + "\n")
    return out
