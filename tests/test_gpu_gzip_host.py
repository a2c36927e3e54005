"""The host side of `--gpu-gzip` without a GPU: pipeline.SplitSink and step B's write_clean over an engine stand-in whose
`deflate` answers with BGZF made on the host (zlib, a member at a time), the flag's rules, and vk_deflate_bound's
arithmetic.  Unmarked: nothing here touches a device."""
import ctypes as C
import gzip
import struct
import zlib
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_write_splits_host import HostText, RefEngine, batch, sample
from varkoder_amd import _capi, cli, pipeline

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def host_bgzf(text):
    out = b""
    for at in range(0, len(text), 65280):
        t = text[at:at + 65280]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = c.compress(t) + c.flush()
        out += (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body +
                struct.pack("<II", zlib.crc32(t), len(t)))
    return out + EOF


class HostBytes(HostText):
    """HostText that can be cut, as the callers cut a device tensor before they copy it back"""

    def __getitem__(self, key):
        return HostBytes(self.a[key])


class GzEngine(RefEngine):
    """RefEngine with ImageEngine.deflate; remembers what it was asked to compress"""

    def __init__(self):
        self.deflated = []

    def deflate(self, text, offs, lens):
        assert all(int(o) % 16 == 0 for o in offs)
        files = [host_bgzf(t) for t in self._texts(text, offs, lens)]
        self.deflated += [int(n) for n in lens]
        oo, at = [], 0
        for f in files:
            oo.append(at)
            at += (len(f) + 15) // 16 * 16
        out = np.zeros(at, dtype=np.uint8)
        for o, f in zip(oo, files):
            out[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        return HostBytes(out), np.array(oo, dtype=np.uint64), np.array([len(f) for f in files], dtype=np.uint64)


class RecordingPool(ThreadPoolExecutor):
    """a pool that notes the bytes of every job's payload"""

    def __init__(self, n):
        super().__init__(n)
        self.payloads = []

    def submit(self, fn, *args, **kw):
        self.payloads += [bytes(a) for a in args if isinstance(a, (bytes, np.ndarray))]
        return super().submit(fn, *args, **kw)


def run_splits(tmp_path, gpu_gzip, pool):
    texts = [sample(11, 60), sample(12, 30)]
    names = ["sA", "sB"]
    text, offs, lens = batch(texts)
    eng = GzEngine()
    stats = OrderedDict()
    sink = pipeline.PngSink(tmp_path / "png", pool, 7, "cgr", {}, {}, 0)
    splits = pipeline.SplitSink(tmp_path / "split_fastqs", pool, overwrite=False, gpu_gzip=gpu_gzip)
    pipeline._ladder_images(eng, text, offs, lens, names, names, 0.0, sink, stats, {"sA": 3, "sB": 4}, splits=splits,
                            no_image=True, min_bp=2000, max_bp=5000, is_query=False)
    splits.finish()
    sink.finish(stats)
    return eng, stats, {f.name: f.read_bytes() for f in (tmp_path / "split_fastqs").iterdir()}


def test_split_sink_hands_the_pool_compressed_bytes_only(tmp_path):
    with RecordingPool(2) as pool:
        _, stats0, plain = run_splits(tmp_path / "host", False, pool)
    with RecordingPool(2) as pool:
        eng, stats1, packed = run_splits(tmp_path / "gpu", True, pool)
        payloads = pool.payloads
    assert sorted(plain) == sorted(packed) == ["sA@00000002K.fq.gz", "sA@00000005K.fq.gz", "sB@00000002K.fq.gz", "sB@00000005K.fq.gz"]
    for name in plain:
        assert gzip.decompress(packed[name]) == gzip.decompress(plain[name]), name
        assert packed[name].endswith(EOF) and packed[name] in payloads, name     # written as it came from the engine
    assert len(eng.deflated) == 4 and sorted(eng.deflated) == sorted(len(gzip.decompress(b)) for b in plain.values())
    assert all(p.startswith(b"\x1f\x8b") for p in payloads)                      # no text went to the pool
    assert {s: v["splitting_bp_per_file"] for s, v in stats0.items()} == {s: v["splitting_bp_per_file"] for s, v in stats1.items()}


def test_pending_bytes_count_what_was_copied_back(tmp_path):
    class Sink(pipeline.SplitSink):
        seen = []

        def _drain(self, room):
            self.seen.append(sum(n for _, n in self.pending))
            super()._drain(room)

    texts = [sample(31, 60)]
    text, offs, lens = batch(texts)
    with ThreadPoolExecutor(1) as pool:
        for gz in (False, True):
            Sink.seen = []
            s = Sink(tmp_path / str(gz), pool, False, gpu_gzip=gz)
            eng = GzEngine()
            recs = pipeline._ladder_plans(eng, text, offs, lens, ["s"], min_bp=2000, max_bp=5000, is_query=False)
            s.emit(eng, text, offs, lens, ["s"], recs, {}, min_bp=2000, max_bp=5000, is_query=False)
            waiting = sum(n for _, n in s.pending)
            s.finish()
            size = sum(f.stat().st_size for f in (tmp_path / str(gz)).iterdir())
            if gz:   # the files' own bytes (each rounded up to 16), not their text
                assert size <= waiting < size + 16 * 2 + 1
            else:
                assert waiting > 2 * size


def test_a_file_gets_its_name_when_whole_and_a_failed_write_surfaces(tmp_path):
    path = tmp_path / "sD@00000002K.fq.gz"
    with pytest.raises(TypeError):
        pipeline.SplitSink._write(path, None, True)
    assert not path.exists()
    pipeline.SplitSink._write(path, host_bgzf(b"@r\nAC\n+\nII\n"), True)
    assert gzip.decompress(path.read_bytes()) == b"@r\nAC\n+\nII\n" and [f.name for f in tmp_path.iterdir()] == [path.name]

    texts = [sample(41, 60)]
    text, offs, lens = batch(texts)
    blocked = tmp_path / "blocked"
    with ThreadPoolExecutor(1) as pool:
        s = pipeline.SplitSink(blocked, pool, False, gpu_gzip=True)
        eng = GzEngine()
        recs = pipeline._ladder_plans(eng, text, offs, lens, ["s"], min_bp=2000, max_bp=5000, is_query=False)
        # a directory stands where a file is to be named: the write fails on the pool, finish() raises it
        (blocked / "s@00000002K.fq.gz").mkdir()
        s.emit(eng, text, offs, lens, ["s"], recs, {}, min_bp=2000, max_bp=5000, is_query=False)
        with pytest.raises(OSError):
            s.finish()


class CleanEngine(GzEngine):
    """step B's calls, answered on the host: a sample's cleaned text is its files' text"""

    def upload_files(self, paths, pool=None):
        return batch([p.read_bytes() for p in paths])

    def clean(self, dev, offs, lens, records, roles, owner, nsamples, **kw):
        texts = [b"".join(t for t, o in zip(self._texts(dev, offs, lens), owner) if o == j) for j in range(nsamples)]
        out, oo, ol = batch(texts)
        stats = np.zeros((nsamples, _capi.VK_CL_NSTAT), dtype=np.uint64)
        stats[:, 162:202] = 1
        return HostBytes(out.a), oo, ol, stats, np.zeros(nsamples, dtype=np.uint32)


def run_clean(tmp_path, gpu_gzip, pool):
    raw = tmp_path / "raw"
    raw.mkdir(parents=True)
    plans = []
    for j, s in enumerate(("sA", "sB")):
        f = raw / (s + ".fq")
        f.write_bytes(sample(50 + j, 40))
        plans.append((s, [(f, _capi.VK_CL_ROLE_UNPAIRED)]))
    eng = CleanEngine()
    opt = pipeline.Cleaning((10, 10), True, True, True, None, False, tmp_path / "clean_reads", None, gpu_gzip)
    writes, stats, base_sd = [], OrderedDict(), {}
    got = list(pipeline._clean_batches(eng, plans, pool, writes, stats, base_sd, opt, 1 << 30, False))
    for w in writes:
        w.result()
    assert len(got) == 1 and got[0][3] == ["sA", "sB"]
    return eng, {s: (raw / (s + ".fq")).read_bytes() for s, _ in plans}, stats


def test_write_clean_writes_what_the_engine_compressed(tmp_path):
    with RecordingPool(2) as pool:
        eng, texts, stats = run_clean(tmp_path / "gpu", True, pool)
        payloads = pool.payloads
    with RecordingPool(2) as pool:
        eng0, _, stats0 = run_clean(tmp_path / "host", False, pool)
        payloads0 = pool.payloads
    assert eng0.deflated == [] and sorted(payloads0) == sorted(texts.values())      # the default path: text to the pool's gzip
    assert sorted(eng.deflated) == sorted(len(t) for t in texts.values())
    assert all(p.startswith(b"\x1f\x8b") for p in payloads) and len(payloads) == 2   # only compressed bytes reach the pool
    for s, t in texts.items():
        for d in ("gpu", "host"):
            assert gzip.decompress((tmp_path / d / "clean_reads" / (s + ".fq.gz")).read_bytes()) == t
            assert (tmp_path / d / "clean_reads" / (s + "_fastp_gpu.json")).is_file()
        assert (tmp_path / "gpu" / "clean_reads" / (s + ".fq.gz")).read_bytes() == host_bgzf(t)
    assert list(stats) == list(stats0) and all("cleaning_time" in v for v in stats.values())


def test_the_flag_goes_only_where_a_fq_gz_is_written(capsys):
    for argv, said in ((["image", "in", "--gpu-gzip"], "only with --from-raw and -i/--int-folder, or with --write-splits"),
                       (["image", "--from-raw", "in", "--gpu-gzip"], "only with --from-raw and -i/--int-folder, or with --write-splits"),
                       (["image", "--from-clean", "in", "-i", "int", "--gpu-gzip"], "only with --from-raw and -i/--int-folder, or with --write-splits"),
                       (["query", "in", "out", "-l", "m", "--vocab", "v", "--gpu-gzip"], "only with --from-raw and -i/--int-folder"),
                       (["query", "--from-raw", "in", "out", "-l", "m", "--vocab", "v", "--gpu-gzip"], "only with --from-raw and -i")):
        with pytest.raises(SystemExit) as err:
            cli.parse_args(argv)
        assert err.value.code == 2
        assert "--gpu-gzip: " + said in capsys.readouterr().err
    assert cli.parse_args(["image", "--from-raw", "in", "-i", "int", "--gpu-gzip"]).gpu_gzip
    assert cli.parse_args(["image", "--from-clean", "in", "-i", "int", "--write-splits", "--gpu-gzip"]).gpu_gzip
    assert cli.parse_args(["query", "--from-raw", "in", "out", "-i", "int", "-l", "m", "--vocab", "v", "--gpu-gzip"]).gpu_gzip
    assert not hasattr(cli.parse_args(["image", "--from-raw", "in", "-i", "int"]), "gpu_gzip")


def test_the_bound_is_members_times_31_plus_the_text_plus_28():
    L = _capi.lib()
    u64 = C.POINTER(C.c_uint64)

    def bound(lens):
        a = np.array(lens, dtype=np.uint64)
        b = C.c_uint64()
        assert L.vk_deflate_bound(a.ctypes.data_as(u64), len(a), C.byref(b)) == _capi.VK_OK
        return b.value

    assert [bound([n]) for n in (0, 1, 65280, 65281)] == [32, 64, 65344, 65376]   # 28; 60; 65,339; 65,371: each rounded up to 16
    assert bound([0, 1, 65280, 65281]) == 32 + 64 + 65344 + 65376 and bound([]) == 0
    assert L.vk_deflate_bound(None, 1, C.byref(C.c_uint64())) == _capi.VK_EINVAL
    assert L.vk_deflate_bound(np.zeros(1, dtype=np.uint64).ctypes.data_as(u64), 1, None) == _capi.VK_EINVAL
