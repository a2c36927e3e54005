"""The host side of `image --write-splits` without a GPU: the flag's rules, and subsample.ladder_files /
pipeline.SplitSink over an engine that answers from tests/ladder_emit_ref.py and the oracle."""
import gzip
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ladder_emit_ref as R
from oracle import oracle
from varkoder_amd import cli, pipeline, subsample


class HostText:
    """a uint8 array where the engine's callers expect a device tensor"""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class RefEngine:
    """read_index, clean_lines and ladder_emit as ImageEngine gives them, computed on the host"""
    k = 7

    def _texts(self, text, offs, lens):
        return [text.a[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]

    def read_index(self, text, offs, lens, parts=0):
        ts = self._texts(text, offs, lens)
        sites = [oracle.count_fastq_sampled(t, 5, 0, 0)[3][0] for t in ts]
        return np.array(sites, dtype=np.uint64), np.array([R.framing_status(t) for t in ts], dtype=np.uint32)

    def clean_lines(self, text, offs, lens):
        return np.array([t.count(b"\n") for t in self._texts(text, offs, lens)], dtype=np.uint64)

    def ladder_emit(self, text, offs, lens, step_sample, step_seed, step_threshold, step_whole, records=None):
        ts = self._texts(text, offs, lens)
        assert list(records) == [(t.count(b"\n") + 1) // 4 for t in ts]
        bodies = [R.emit_ref(ts[i], int(s), int(t), bool(w)) for i, s, t, w in zip(step_sample, step_seed, step_threshold, step_whole)]
        out_offs, at = [], 0
        for b in bodies:
            out_offs.append(at)
            at += (len(b) + 15) // 16 * 16
        out = np.zeros(at + 64, dtype=np.uint8)
        for o, b in zip(out_offs, bodies):
            out[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        return (HostText(out), np.array(out_offs, dtype=np.uint64), np.array([len(b) for b in bodies], dtype=np.uint64),
                np.zeros(len(ts), dtype=np.uint32))


def batch(texts):
    offs, at = [], 0
    for t in texts:
        offs.append(at)
        at += (len(t) + 15) // 16 * 16
    buf = np.zeros(at + 16, dtype=np.uint8)
    for o, t in zip(offs, texts):
        buf[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
    return HostText(buf), np.array(offs, dtype=np.uint64), np.array([len(t) for t in texts], dtype=np.uint64)


def sample(seed, reads):
    import random
    rng = random.Random(seed)
    return "".join("@s%d.%d\n%s\n+\n%s\n" % (seed, i, "".join(rng.choice("ACGT") for _ in range(n)), "F" * n)
                   for i, n in enumerate(rng.choice((150, 150, 700)) for _ in range(reads))).encode()


def test_ladder_files_follow_the_counting_plan_in_any_slicing():
    texts = [sample(1, 60), sample(2, 20), b"@broken\nAC\n", sample(3, 4)]
    text, offs, lens = batch(texts)
    eng = RefEngine()
    nsites, status = eng.read_index(text, offs, lens)
    found = {}
    for slice_bytes in (1 << 30, 500):
        got = {}
        for dev, steps in subsample.ladder_files(eng, text, offs, lens, nsites, status, seed=5, min_bp=2000, max_bp=None,
                                                 slice_bytes=slice_bytes):
            host = dev.cpu().numpy()
            for i, bp, o, n in steps:
                got[(i, bp)] = host[o:o + n].tobytes()
        found[slice_bytes] = got
    assert found[500] == found[1 << 30]
    _, plans = subsample.ladder_plan(nsites, status, 2000, None)
    assert plans[2] == [] and plans[3] == [] and len(plans[0]) >= 3      # bad framing; too little data
    want = {(i, bp): R.emit_ref(texts[i], seed, thr, whole) for i, _, bp, seed, thr, whole in subsample.plan_steps(plans, nsites, 5)}
    assert found[500] == want and all(k[0] in (0, 1) for k in want)
    # a whole first step and seed + level behind it
    assert want[(0, plans[0][0])] == R.emit_ref(texts[0], 5, 0, whole=True)
    assert want[(0, plans[0][1])] == R.emit_ref(texts[0], 6, subsample.threshold(plans[0][1], nsites[0]))


def test_split_sink_writes_gzip_files_and_keeps_complete_samples(tmp_path):
    texts = [sample(11, 60), sample(12, 30)]
    names = ["sA", "sB"]
    text, offs, lens = batch(texts)
    eng = RefEngine()
    with ThreadPoolExecutor(2) as pool:
        stats = OrderedDict()
        sink = pipeline.PngSink(tmp_path / "png", pool, 7, "cgr", {}, {}, 0)
        splits = pipeline.SplitSink(tmp_path / "int" / "split_fastqs", pool, overwrite=False)
        ladder = dict(min_bp=2000, max_bp=5000, is_query=False)
        pipeline._ladder_images(eng, text, offs, lens, names, names, 0.0, sink, stats, {"sA": 3, "sB": 4}, splits=splits,
                                no_image=True, **ladder)
        splits.finish()
        sink.finish(stats)
        files = sorted((tmp_path / "int" / "split_fastqs").iterdir())
        assert [f.name for f in files] == ["sA@00000002K.fq.gz", "sA@00000005K.fq.gz", "sB@00000002K.fq.gz", "sB@00000005K.fq.gz"]
        nsites, _ = eng.read_index(text, offs, lens)
        for j, (s, seed) in enumerate((("sA", 3), ("sB", 4))):
            assert stats[s]["splitting_bp_per_file"] == "5000,2000" and "7mer_counting_time" not in stats[s]
            for level, bp in enumerate((5000, 2000)):
                body = gzip.decompress((tmp_path / "int" / "split_fastqs" / (subsample.split_name(s, bp) + ".fq.gz")).read_bytes())
                assert body == R.emit_ref(texts[j], seed + level, subsample.threshold(bp, nsites[j]))
        assert not list((tmp_path / "png").rglob("*.png"))
        # one file of sB gone: sB is written again, sA is left alone
        files[2].unlink()
        before = {f: f.stat().st_mtime_ns for f in files if f.exists()}
        pipeline._ladder_images(eng, text, offs, lens, names, names, 0.0, sink, OrderedDict(), {"sA": 3, "sB": 4}, splits=splits,
                                no_image=True, **ladder)
        splits.finish()
        assert files[2].exists()
        assert all(f.stat().st_mtime_ns == t for f, t in before.items() if f.name.startswith("sA@"))


class RefusingEngine(RefEngine):
    """an emit that refuses one sample's framing although the read index passed it"""

    def __init__(self, refused):
        self.refused = refused

    def ladder_emit(self, text, offs, lens, step_sample, *rest, **kw):
        out, oo, ol, st = super().ladder_emit(text, offs, lens, step_sample, *rest, **kw)
        mine = [i for i, t in enumerate(self._texts(text, offs, lens)) if t == self.refused]
        st[mine] = 4
        ol[[j for j, i in enumerate(step_sample) if i in mine]] = 0
        return out, oo, ol, st


def test_a_sample_the_emit_refuses_fails_alone_and_a_file_is_named_when_whole(tmp_path):
    texts = [sample(21, 60), sample(22, 60), sample(23, 60)]
    names = ["sA", "sB", "sC"]
    text, offs, lens = batch(texts)
    eng = RefusingEngine(texts[1])
    nsites, status = eng.read_index(text, offs, lens)
    with pytest.raises(RuntimeError):   # (without a place to put it the disagreement is an error)
        list(subsample.ladder_files(eng, text, offs, lens, nsites, status, min_bp=2000, max_bp=5000))
    with ThreadPoolExecutor(2) as pool:
        stats = OrderedDict()
        sink = pipeline.PngSink(tmp_path / "png", pool, 7, "cgr", {}, {}, 0)
        splits = pipeline.SplitSink(tmp_path / "split_fastqs", pool, overwrite=False)
        splits.MAX_PENDING_BYTES = 0   # (every slice waits for the one before it)
        pipeline._ladder_images(eng, text, offs, lens, names, names, 0.0, sink, stats, {}, splits=splits, no_image=True,
                                min_bp=2000, max_bp=5000, is_query=False)
        splits.finish()
        sink.finish(stats)
    assert stats["sB"] == {"failed_step": "split"}
    assert stats["sA"]["splitting_bp_per_file"] == stats["sC"]["splitting_bp_per_file"] == "5000,2000"
    assert sorted(f.name for f in (tmp_path / "split_fastqs").iterdir()) == [
        "sA@00000002K.fq.gz", "sA@00000005K.fq.gz", "sC@00000002K.fq.gz", "sC@00000005K.fq.gz"]   # (and no .part left)
    # a write that dies leaves no file under the final name
    broken = tmp_path / "split_fastqs" / "sD@00000002K.fq.gz"
    with pytest.raises(TypeError):
        pipeline.SplitSink._write(broken, None)
    assert not broken.exists()


def test_the_flag_needs_its_entry_and_its_folder(capsys):
    """(the message tells the flag's own rule from argparse's unknown flag, which exits with 2 as well)"""
    for argv, said in ((["image", "in", "--write-splits", "-i", "int"], "only with --from-raw or --from-clean"),
                       (["image", "--from-clean", "in", "--write-splits"], "needs -i"),
                       (["image", "--from-raw", "in", "--write-splits"], "needs -i")):
        with pytest.raises(SystemExit) as err:
            cli.parse_args(argv)
        assert err.value.code == 2
        assert "--write-splits: " + said in capsys.readouterr().err
    args = cli.parse_args(["image", "--from-clean", "in", "-i", "int", "--write-splits", "-X", "-x"])
    opts = cli.split_options(args)
    assert str(opts["split_dir"]).endswith("int/split_fastqs") and opts["overwrite"] and opts["no_image"]
    assert cli.split_options(cli.parse_args(["image", "--from-clean", "in", "-i", "int", "-X"])) == {}
