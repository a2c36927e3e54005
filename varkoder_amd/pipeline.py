"""Batched steps D+E of run_clean2img (commands/image.py:1054-1127) for already cleaned and
split FASTQ files: many files per launch, images written by a host thread pool, optional
sharding over the ranks of a torch.distributed job.

Steps B/C of the reference (fastp, reformat.sh) are external tools that are out of this
path's scope; this module enters where the reference enters step D: with
files named `<sample>@<bp>K.fq[.gz]` as split_fastq leaves them (image.py:699-709).
"""
import os
import time
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from .config import QUAL_THRESH, SAMPLE_BP_SEP
from .image import counts_name, eprint, png_head, png_name, shard_folder, stem, write_png, write_png_parts
from .shard import TailQueue, agreed_weights, file_weights, gz_text_bytes, shard_by_size, split_head_tail


# Text bytes in HBM per batch.  Plain files: small enough that reading the next batch from disk overlaps
# the copy of this one.  gzip files are inflated on the GPU, which wants many files in flight, and their
# staging is cheap: larger batches.  The first batch of a run is cut short so that the device has work
# while the bulk of the files is still being read.  (bench.py's end-to-end leg runs with these defaults.)
DEFAULT_BATCH_BYTES = 2 << 30
DEFAULT_GZ_BATCH_BYTES = 16 << 30
FIRST_BATCH_BYTES = 512 << 20


def image_name(fastq_path, k, mapping_code):
    """`<sample>@<bp>K+<mapping>+k<k>.png` straight from a split FASTQ's name."""
    return png_name(counts_name(fastq_path, k), mapping_code)


class RouteChooser:
    """Plain-text files reach HBM by one of two routes (engine.plain_route): STAGED -- the I/O threads read() them into a
    pinned buffer, one DMA per batch -- or MAPPED -- the files' page-cache pages are mapped and the GPU copies out of
    them, no read() at all.  Which is faster depends on the host: with 16 fast cores the staged route runs at the link's
    rate (BENCH_r04: 56 of 57.6 GB/s); on a slower host the read() copies -- and the memory bandwidth they take from the DMA
    -- hold it at 44 (BENCH_r05).  So the run measures itself: three batches on the route it starts with (behind two that
    do not count); if they moved less than 85 % of what the link carries (measured once, 128 MiB pinned -> device), the
    same on the other route, and the rest on whichever was faster.  VARKODER_AMD_MMAP=0/1 pins the route and switches this off."""

    def __init__(self, eng, tm):
        from . import engine as E
        self.eng, self.tm, self.E = eng, tm, E
        self.on = E.USE_MAPPED_UPLOAD is None and getattr(eng, "route_override", None) is None and hasattr(eng, "h2d_link_rate")
        if getattr(eng, "route_rates", None):    # (an earlier pass of this engine measured and chose: say so in this pass's record)
            tm["plain_route_rates_gb_s"] = dict(eng.route_rates)
        self.rate = {}          # route -> [plain bytes, seconds, batches] over the batches that count
        self.seen = {}          # route -> batches seen
        self.first = None       # the route the run began on
        self.trial = False      # the other route is being tried

    def batch_done(self, bi, staged, seconds):
        if not isinstance(staged, dict) or "disk" not in staged:
            return
        route = staged.get("plain_route", "staged")   # (as stage_files brought this batch in)
        self.tm["plain_route"] = route
        if not self.on:
            return
        plain = int(staged["disk"][~staged["is_gz"]].sum()) if len(staged["disk"]) else 0
        if plain == 0:
            return
        # the first batches of a route do not count: the run's short first batch, the pinned staging buffers growing to
        # their size, the first registrations of mapped pages (BENCH r06, first cut: 21.8 GB/s "measured" for the staged route
        # in a pass that then ran at 51)
        self.seen[route] = self.seen.get(route, 0) + 1
        if self.seen[route] <= (3 if not self.trial else 2):   # (batch 0 is short; each of the two staging buffers grows once more after it)
            return
        acc = self.rate.setdefault(route, [0, 0.0, 0])
        acc[0] += plain
        acc[1] += seconds
        acc[2] += 1
        if self.first is None:
            self.first = route
        other = "staged" if self.first == "mapped" else "mapped"
        if not self.trial:
            if route == self.first and acc[2] >= 3:
                link = self.eng.h2d_link_rate()
                got = acc[0] / acc[1]
                self.tm["plain_route_rates_gb_s"] = {route: got / 1e9, "link": link / 1e9}
                if got < 0.85 * link:
                    self.eng.route_override = other
                    self.trial = True
                else:
                    self.eng.route_override = route   # (settled: later passes of this engine do not measure again)
                    self.tm["plain_route_rates_gb_s"]["chosen"] = route
                    self.on = False
                self.eng.route_rates = dict(self.tm["plain_route_rates_gb_s"])
        elif route == other and acc[2] >= 3:
            a, b = self.rate[self.first], self.rate[other]
            best = other if b[0] / b[1] > a[0] / a[1] else self.first
            self.eng.route_override = best
            self.tm["plain_route_rates_gb_s"].update({other: b[0] / b[1] / 1e9, "chosen": best})
            self.eng.route_rates = dict(self.tm["plain_route_rates_gb_s"])
            self.on = False


def text_bytes(path):
    """Text bytes of a read file as it lies in HBM (a gzip file counts the text its framing names, shard.gz_text_bytes:
    it is inflated on the GPU)."""
    path = Path(path)
    return gz_text_bytes(path) if path.suffix == ".gz" else os.path.getsize(path)


def batches(items, limit, size=text_bytes, first_limit=None):
    """Pack `items` greedily, in order, into batches of at most `limit` bytes by size(item); the first batch at most
    min(limit, first_limit).  An item joins the batch unless the batch is non-empty and would pass its limit: an item
    larger than the limit gets a batch of its own, a batch that lands exactly on the limit is not split.  Yields
    (batch, its bytes, the time it was begun: before its items are sized, except the first of a later batch)."""
    cap = limit if first_limit is None else min(limit, first_limit)
    batch, nbytes, t0 = [], 0, time.perf_counter()
    for item in items:
        sz = size(item)
        if batch and nbytes + sz > cap:
            yield batch, nbytes, t0
            batch, nbytes, cap, t0 = [], 0, limit, time.perf_counter()
        batch.append(item)
        nbytes += sz
    if batch:
        yield batch, nbytes, t0


@contextmanager
def engine_scope(engine, k, mapping_code, device, io_threads):
    """(engine, host thread pool) of one entry point: `engine`, or one made here and closed here, once.  An error
    inside must not leave the pool writing files into outdir behind the caller's back: queued work is cancelled
    when an exception leaves, and what runs is waited for either way."""
    from .engine import ImageEngine
    eng = engine or ImageEngine(k=k, mapping=mapping_code, device=device)
    pool = ThreadPoolExecutor(io_threads)
    failed = True
    try:
        yield eng, pool
        failed = False
    finally:
        pool.shutdown(wait=True, cancel_futures=failed)
        if engine is None:
            eng.close()


class PngSink:
    """Where an entry point's images go: the output folder (made here) with its md5 sub-folders, the text chunks'
    sources (labels and base_sd by sample; base_sd may still be filling), the pool that writes and what it has pending.
    encoder: None, or the engine whose png() makes the files' IDAT chunks on the GPU (--gpu-png): the pool's job is then
    the file's head (image.png_head) and the write."""

    def __init__(self, outdir, pool, k, mapping_code, labels, base_sd, subfolder_levels, encoder=None):
        self.outdir, self.pool, self.k, self.mapping_code = Path(outdir), pool, k, mapping_code
        self.labels, self.base_sd, self.subfolder_levels, self.encoder = labels, base_sd, subfolder_levels, encoder
        self.pending = []
        self.outdir.mkdir(parents=True, exist_ok=True)

    def path(self, name):
        return shard_folder(self.outdir, name, self.subfolder_levels) / name

    def rows(self, img):
        """What submit takes for each image of a batch's device tensor img [n, side, side], handed over once: the host
        arrays, or with an encoder the images' IDAT chunks (rows of failed samples are encoded and never asked for)."""
        if len(img) == 0:
            return []
        return self.encoder.png(img) if self.encoder is not None else img.cpu().numpy()

    def submit(self, key, sample, name, arr):
        """Queue image `arr` (a row of rows()) of `sample` as file `name`; its writing time goes to stats row `key` (finish)."""
        path = self.path(name)
        path.parent.mkdir(parents=True, exist_ok=True)
        text = (self.labels.get(sample, []), self.base_sd.get(sample, 0), QUAL_THRESH, self.mapping_code)
        if isinstance(arr, bytes):
            job = self.pool.submit(self._write_parts, path, arr, *text)
        else:
            job = self.pool.submit(write_png, arr.copy(), path, *text)
        self.pending.append((key, time.perf_counter(), job))

    def _write_parts(self, path, idat, *text):
        write_png_parts(path, png_head(self.encoder.side, *text), idat)

    def finish(self, stats):
        """Wait for every image (a failed write raises here) and add `k<k>_img_time` to its stats row."""
        key = "k" + str(self.k) + "_img_time"
        for row, t, fut in self.pending:
            fut.result()
            stats[row][key] = stats[row].get(key, 0) + (time.perf_counter() - t)


def sample_weights(samples, world):
    """Work estimate of each of samples = [(sample, [files])]: the sum of its files' weights, as every rank uses them
    (shard.agreed_weights: a collective) when world > 1.  No samples: [] and no collective."""
    every = [f for _, files in samples for f in files]
    fw = (agreed_weights(every) if world > 1 else file_weights(every)) if every else []
    weights, at = [], 0
    for _, files in samples:
        weights.append(sum(fw[at:at + len(files)]))
        at += len(files)
    return weights


def fastqs_to_images(files, outdir, k=7, mapping_code="cgr", labels=None, base_sd=None, overwrite=False,
                     subfolder_levels=0, device=0, rank=0, world=1, batch_bytes=None, io_threads=8,
                     engine=None, verbose=False, timings=None, weights=None, tail_frac=0.1, gpu_png=False):
    """Process this rank's share of `files`.  Returns {sample_file_stem: OrderedDict(stats)}
    with the reference's stats keys `<k>mer_counting_time` and `k<k>_img_time` (per-file
    share of the batch wall time) or `failed_step` for files whose FASTQ framing is bad.
    batch_bytes: None = DEFAULT_BATCH_BYTES (DEFAULT_GZ_BATCH_BYTES when every file is gzip).
    weights: the files' work estimates as every rank of the job uses them (shard.agreed_weights -- a collective: pass them in
    when this call sits in a try block that a failing rank would leave early); None: agreed on here.
    timings: optional dict that receives where this thread's wall time went (seconds): waiting for the
    staging thread (`stage_wait_s`), the copy to the device and the inflate (`upload_s`, of which
    `inflate_s`), kernels + copies back (`kernels_s`) and waiting for the last hand-overs and PNGs (`png_tail_s`);
    `png_submit_s` = handing images to the PNG pool, on a thread of its own since round 5 (not this thread's time); `batches`.
    gpu_png: the files' IDAT chunks are made on the GPU (ImageEngine.png) and the pool only writes."""
    files = [Path(f) for f in files]
    if weights is None:   # (a collective only when this call itself is one rank's share of a job: bench.py's per-rank legs call with world = 1 inside a group)
        weights = agreed_weights(files) if world > 1 else file_weights(files)
    # Size-aware (rank 0's view of the sizes: shard.agreed_weights).  With a process group, the longest files -- nine tenths
    # of the weight -- are dealt statically, and the many small ones at the end of the order are pulled from a shared
    # cursor by whichever rank gets there first (shard.split_head_tail, TailQueue): the deal balances estimates, the
    # tail what they got wrong.  (The queue is made here, before anything a single rank could fail in: every rank
    # constructs it, none has to reach it.)
    import torch.distributed as dist
    grouped = world > 1 and dist.is_available() and dist.is_initialized() and dist.get_world_size() == world
    head, tail = split_head_tail(weights, tail_frac if grouped else 0.0)
    mine = [files[head[j]] for j in shard_by_size([weights[i] for i in head], rank, world)]
    tail_files = [files[i] for i in tail]
    tail_queue = TailQueue(len(tail_files)) if tail_files else None
    tail_chunk = max(1, len(tail_files) // (6 * world))   # files per claim: ~6 claims per rank
    stats = OrderedDict()
    tm = timings if timings is not None else {}
    for key in ("stage_wait_s", "upload_s", "inflate_s", "kernels_s", "png_submit_s", "png_tail_s"):
        tm.setdefault(key, 0.0)
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        sink = PngSink(outdir, pool, k, mapping_code, labels or {}, base_sd or {}, subfolder_levels, eng if gpu_png else None)

        def wanted(fs):
            out = []
            for f in fs:
                if not overwrite and sink.path(image_name(f, k, mapping_code)).is_file():
                    eprint("File exists. Skipping image for file:", str(f))
                    continue
                out.append(f)
            return out

        todo = wanted(mine)
        if batch_bytes is None:
            every = todo + tail_files
            batch_bytes = DEFAULT_GZ_BATCH_BYTES if every and all(f.suffix == ".gz" for f in every) else DEFAULT_BATCH_BYTES

        def batch_source():
            """This rank's batches by text size in HBM: its static share first (the first batch cut short), then what it
            claims of the tail, a chunk per batch."""
            for batch, nbytes, _ in batches(todo, batch_bytes, first_limit=FIRST_BATCH_BYTES):
                yield batch, nbytes
            while tail_queue is not None:
                got = tail_queue.next(tail_chunk)
                if len(got) == 0:
                    break
                batch = wanted([tail_files[i] for i in got])
                tm["tail_files"] = tm.get("tail_files", 0) + len(batch)
                if batch:
                    yield batch, sum(text_bytes(f) for f in batch)
        # The host half of a batch (file reads into a pinned buffer) runs one batch ahead on its own
        # thread, into the other of two staging buffers, while this thread copies and processes.
        stager = ThreadPoolExecutor(1)
        finisher, handed = ThreadPoolExecutor(1), []
        done = False
        chooser = RouteChooser(eng, tm)
        try:
            source = batch_source()
            cur = next(source, None)
            staged = stager.submit(eng.stage_files, cur[0], pool, 0) if cur else None
            bi = -1
            while cur is not None:
                bi += 1
                batch, nbytes = cur
                t0 = time.perf_counter()
                ready = staged.result()
                tm["stage_wait_s"] += time.perf_counter() - t0
                cur = next(source, None)          # (a chunk of the tail is claimed here: one batch ahead, like the staging)
                if cur is not None:
                    staged = stager.submit(eng.stage_files, cur[0], pool, (bi + 1) & 1)
                for h in handed:   # a hand-over that failed (a folder that cannot be made) stops the pass here, not after the last batch
                    if h.done() and h.exception() is not None:
                        raise h.exception()
                tu = time.perf_counter()
                dev, offs, lens = eng.upload_staged(ready, timings=tm)
                t1 = time.perf_counter()
                tm["upload_s"] += t1 - tu
                img, hist, status = eng.fastq_to_images(dev, offs, lens)
                st = status.cpu().numpy()
                imgs = sink.rows(img)
                nz = (hist != 0).any(dim=1).cpu().numpy()
                t2 = time.perf_counter()
                tm["kernels_s"] += t2 - t1
                chooser.batch_done(bi, ready, t2 - t0)

                def hand_over(batch=batch, st=st, imgs=imgs, nz=nz, per_file=(t2 - t0) / len(batch)):
                    # stats rows and PNG jobs of one batch: on a thread of its own (batches in order), beside the next batch's
                    # upload and inflate, in whose C calls this thread's interpreter lock is free (9 % of a .fq.gz pass before)
                    th = time.perf_counter()
                    for j, f in enumerate(batch):
                        key = stem(f)
                        s = stats.setdefault(key, OrderedDict())
                        if st[j] or not nz[j]:
                            eprint("K-MER COUNTING FAIL, SKIPPING FILE:", f)
                            s["failed_step"] = "image"
                            continue
                        s[str(k) + "mer_counting_time"] = per_file
                        sink.submit(key, key.split("@")[0], image_name(f, k, mapping_code), imgs[j])
                    tm["png_submit_s"] += time.perf_counter() - th   # (this thread's time: off the main thread's path)

                handed.append(finisher.submit(hand_over))
                if verbose:
                    eprint(f"batch of {len(batch)} files, {nbytes} bytes: upload {t1 - t0:.3f}s kernels {t2 - t1:.3f}s")
            tt = time.perf_counter()
            for h in handed:
                h.result()   # (an exception of a batch's hand-over surfaces here)
            sink.finish(stats)
            done = True
        finally:
            # An error anywhere above (a copy that runs out of memory, a PNG that cannot be written) must not leave the staging
            # thread reading the next batch or queued hand-overs writing PNGs into outdir behind the caller's back (the pool's
            # turn comes last, as the scope is left).
            for ex in (stager, finisher):
                ex.shutdown(wait=True, cancel_futures=not done)
        tm["png_tail_s"] += time.perf_counter() - tt
        tm["batches"] = tm.get("batches", 0) + bi + 1
    return stats


def clean_to_images(files, outdir, k=7, mapping_code="cgr", min_bp=50000, max_bp=None, is_query=False, seeds=None,
                    labels=None, base_sd=None, subfolder_levels=0, device=0, rank=0, world=1, batch_bytes=None,
                    io_threads=8, engine=None, verbose=False, weights=None, split_dir=None, overwrite=False, no_image=False,
                    gpu_gzip=False, gpu_png=False, screen=None, qc_dir=None, spectrum=None):
    """Steps C+D+E of run_clean2img (commands/image.py:1006-1127) for cleaned, UNSPLIT read files
    `<sample>.fq[.gz]` (the reference's `<int_folder>/clean_reads/`): the 1-2-5 ladder of subsamples
    is drawn on the GPU (subsample.ladder_counts) instead of writing one file per size with
    reformat.sh, and every step becomes `<sample>@<bp>K+<mapping>+k<k>.png`.

    split_dir: also write every step's reads to `split_dir/<sample>@<bp>K.fq.gz` (SplitSink), as the reference's
    split_fastq leaves them; overwrite: also where a sample's files are all there.  no_image (with split_dir: the
    reference's -X, :1055): stop after step C -- no counting, no PNG.  gpu_gzip: the files are compressed on the GPU
    (SplitSink).  gpu_png: the images' IDAT chunks are made on the GPU (PngSink).  screen (Screen): the uploaded reads are
    screened in HBM before the ladder (`--exclude-fasta` / `--keep-fasta`); the stats gain its three columns.  qc_dir
    (`--qc-report`): `<qc_dir>/<sample>.qc.json` of the uploaded reads (behind the screen), its `after` sections only, and
    qc.columns' columns in the stats.  spectrum (Spectrum, `--kmer-spectrum`): `<dir>/<sample>.spectrum.json` of the
    uploaded reads (behind the screen), counted once per sample, and spectrum.columns' columns in the stats.

    seeds: {sample: int} (default 0).  Returns {sample: OrderedDict(stats)} with the reference's
    keys `splitting_bp_per_file`, `<k>mer_counting_time`, `k<k>_img_time`, or `failed_step`."""
    files = [Path(f) for f in files]
    if weights is None:
        weights = agreed_weights(files) if world > 1 else file_weights(files)   # (a collective when sharded: see fastqs_to_images)
    mine = [files[i] for i in shard_by_size(weights, rank, world)]   # size-aware; rank 0's view of the sizes: see shard.agreed_weights
    stats = OrderedDict()
    if batch_bytes is None:
        batch_bytes = DEFAULT_GZ_BATCH_BYTES if mine and all(f.suffix == ".gz" for f in mine) else DEFAULT_BATCH_BYTES
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        sink = PngSink(outdir, pool, k, mapping_code, labels or {}, base_sd or {}, subfolder_levels, eng if gpu_png else None)
        splits = SplitSink(split_dir, pool, overwrite, gpu_gzip) if split_dir is not None else None
        reports = []
        for batch, nbytes, t0 in batches(mine, batch_bytes):
            dev, offs, lens = eng.upload_files(batch, pool)
            if screen is not None:
                dev, offs, lens, _ = screen.apply(eng, dev, offs, lens, [stem(f) for f in batch], stats, pool)
            spec_rows = None
            if spectrum is not None:   # (before the qc: with `--depth-filter` the qc and the ladder see what is kept)
                spec_rows = spectrum.after(eng, dev, offs, lens)
                if spectrum.band is not None:
                    spec_rows, dev, offs, lens = spec_rows
            if qc_dir is not None:
                for f, row in zip(batch, QcReport.after(eng, dev, offs, lens)):
                    QcReport(qc_dir).emit(stem(f), None, row, stats.setdefault(stem(f), OrderedDict()), pool, reports)
            if spectrum is not None:
                for f, row in zip(batch, spec_rows):
                    spectrum.emit(stem(f), row, stats.setdefault(stem(f), OrderedDict()), pool, reports)
            t1, t2 = _ladder_images(eng, dev, offs, lens, [stem(f) for f in batch], batch, t0, sink, stats, seeds or {},
                                    splits=splits, no_image=no_image, min_bp=min_bp, max_bp=max_bp, is_query=is_query)
            if verbose:
                eprint(f"batch of {len(batch)} samples, {nbytes} bytes: upload+ladder {t1 - t0:.3f}s images {t2 - t1:.3f}s")
        for w in reports:
            w.result()
        if splits is not None:
            splits.finish()
        sink.finish(stats)
    return stats


@dataclass
class Screen:
    """`--exclude-fasta` / `--keep-fasta`: cleaned reads in HBM are screened against the k-mers of one reference FASTA
    before the ladder sees them ("--exclude-fasta / --keep-fasta: the rule").  The set is built once per
    rank and run, on the first use, and lives with the engine (ImageEngine.screen_sets)."""
    fasta: object
    k: int = 31
    min_hits: int = 1
    keep: bool = False

    def set_on(self, eng, pool=None):
        """The reference's ScreenSet on this engine: the file uploaded (a .gz inflated in HBM) and its set built on
        the first call."""
        sets = eng.__dict__.setdefault("screen_sets", {})
        key = (str(self.fasta), self.k)
        if key not in sets:
            dev, _, lens = eng.upload_files([Path(self.fasta)], pool)
            status = getattr(eng, "last_upload_status", None)
            if status is not None and status[0]:
                raise Exception(f"{self.fasta}: inflate status {int(status[0])}")
            try:
                sets[key] = eng.screen_set(dev, int(lens[0]), self.k)
            except ValueError as e:
                raise Exception(f"{self.fasta}: {e}") from e
        return sets[key]

    def report(self, sset, row):
        """The `"screen"` object of `<sample>_fastp_gpu.json` for a sample's stats row."""
        return {"reference": Path(self.fasta).name, "k": self.k, "min_hits": self.min_hits,
                "mode": "keep" if self.keep else "exclude", "distinct_kmers": sset.distinct, **self.columns(row)}

    @staticmethod
    def columns(row):
        """The columns of stats.csv for a sample's stats row (records in, records kept, bases in, bases kept)."""
        return {"screen_reads_in": int(row[0]), "screen_reads_removed": int(row[0]) - int(row[1]),
                "screen_basepairs_removed": int(row[2]) - int(row[3])}

    def apply(self, eng, text, offs, lens, names, stats, pool=None):
        """The samples `names` in HBM (text[offs[i] .. +lens[i])) screened: (text, offsets, lengths, stats rows) of what
        is kept, laid out as the input was; fills the samples' columns in `stats` ({sample: OrderedDict}, or None).  A
        sample whose framing the screen refuses keeps no reads, and fails where an empty cleaned sample fails."""
        sset = self.set_on(eng, pool)
        out, ooffs, olens, rows, status = eng.screen(text, offs, lens, sset, keep=self.keep, min_hits=self.min_hits)
        for j, s in enumerate(names):
            if status[j]:
                eprint("SCREEN FAIL:", s, "- status", int(status[j]))
            if stats is not None:
                stats.setdefault(s, OrderedDict()).update(self.columns(rows[j]))
        return out, ooffs, olens, rows


@dataclass
class QcReport:
    """`--qc-report DIR`: the reads' quality profiles, counted where their text lies in HBM (ImageEngine.qc; the rule:
    INTEGRATION.md, "--qc-report: the rule") -- the raw texts under the cleaning's read budget and the cleaned text as the
    ladder sees it -- written as `DIR/<sample>.qc.json` (qc.report) with their stats.csv columns (qc.columns)."""
    dir: object

    @staticmethod
    def before(eng, text, offs, lens, records, roles, owner, nsamples):
        """Per sample {"read1" | "read2" | "single": row} of the raw streams in HBM: stream i gives its first records[i]
        records to sample owner[i] as roles[i]; a role's streams are taken together, a role without one has no entry.
        A stream with a status counts as empty (the cleaning fails its sample)."""
        from . import qc
        rows, _ = eng.qc(text, offs, lens, records)
        parts = [dict() for _ in range(nsamples)]
        for i, (role, j) in enumerate(zip(roles, owner)):
            parts[j].setdefault(qc.ROLE_KEYS[int(role)], []).append(rows[i])
        return [{role: qc.add_rows(rs) for role, rs in p.items()} for p in parts]

    @staticmethod
    def after(eng, text, offs, lens):
        """The rows of cleaned samples in HBM, every record counted."""
        return eng.qc(text, offs, lens)[0]

    def emit(self, sample, before, after, stats_row, pool, writes):
        """A sample's file queued on the pool (its future goes to `writes`) and its columns into stats_row (None: none)."""
        from . import qc
        if stats_row is not None:
            stats_row.update(qc.columns(qc.add_rows(before.values()) if before else None, after))
        writes.append(pool.submit(qc.write_report, self.dir, sample, qc.report(before, after)))


@dataclass
class Spectrum:
    """`--kmer-spectrum DIR`: the k-mer spectrum of a sample's cleaned text as the ladder sees it -- behind the screen,
    once per sample, never per ladder step -- counted where the text lies in HBM (ImageEngine.spectrum; the rule:
    INTEGRATION.md, "`--kmer-spectrum`: the rule"), written as `DIR/<sample>.spectrum.json` (spectrum.report) with its
    stats.csv columns (spectrum.columns)."""
    dir: object
    k: int = 21
    every: int = 1
    sketch_size: object = None    # `--spectrum-sketch S`: also `DIR/<sample>.sketch.npy` and the json's "sketch" object
    sketch_min_count: int = 1     # `--spectrum-sketch-min-count M`
    band: object = None           # `--depth-filter LO:HI` (depth.Band): the reads behind the spectrum are those whose median k-mer depth lies in it

    def after(self, eng, text, offs, lens):
        """The rows of cleaned samples in HBM.  A sample the count refuses (its framing) is reported and has a zero row.
        With a sketch size every row comes as (row, the sketch's hashes, its eligible count).

        With a band: (rows, text, offsets, lengths) -- the samples' reads filtered by depth (INTEGRATION.md,
        "`--depth-filter`: the rule"), laid out as the input was, for everything behind the spectrum to see in place of
        the input; every row then comes as (the row as without a band, the depth row, the sample's resolved band)."""
        kw = {}
        if self.sketch_size is not None:
            kw["sketch"] = (self.sketch_size, self.sketch_min_count)
        if self.band is not None:
            kw["depth"] = self.band
        rows, status, *rest = eng.spectrum(text, offs, lens, k=self.k, every=self.every, **kw)
        for j in np.flatnonzero(status):
            eprint("SPECTRUM FAIL: sample", int(j), "of its batch - status", int(status[j]))
        if self.sketch_size is not None:
            hashes, info, *rest = rest
            rows = [(rows[j], hashes[j, :int(info[j, 1])].copy(), int(info[j, 0])) for j in range(len(rows))]
        if self.band is None:
            return rows
        out, ooffs, olens, drows, bands = rest
        for j, b in enumerate(bands):
            if not status[j] and not b[2]:
                eprint("DEPTH FILTER SKIPPED: sample", int(j), "of its batch -", b[3])
        return [(rows[j], drows[j], bands[j]) for j in range(len(rows))], out, ooffs, olens

    def emit(self, sample, row, stats_row, pool, writes):
        """A sample's file queued on the pool (its future goes to `writes`) and its columns into stats_row (None: none)."""
        from . import depth, sketch, spectrum
        sk = dp = None
        if self.band is not None:
            row, drow, band = row
            dp = depth.report(drow, self.band, band[:2], band[2], band[3])
        if self.sketch_size is not None:
            row, hashes, eligible = row
            sk = sketch.meta(self.sketch_size, self.sketch_min_count, eligible, len(hashes))
            writes.append(pool.submit(sketch.write_sketch, self.dir, sample, hashes))
        if stats_row is not None:
            stats_row.update(spectrum.columns(row, self.k, self.every))
            if dp is not None:
                stats_row.update(depth.columns(drow))
        obj = spectrum.report(row, self.k, self.every, sketch=sk)
        if dp is not None:
            obj["depth_filter"] = dp
        writes.append(pool.submit(spectrum.write_report, self.dir, sample, obj))


@dataclass
class GenomeSpectrum:
    """`--from-fasta --genome-spectrum DIR`: the k-mer spectrum of an assembly, counted from the FASTA text where it lies
    in HBM for the image count (ImageEngine.spectrum_fasta; the rule: INTEGRATION.md, "`--genome-spectrum`: the rule"),
    written as `DIR/<sample>.spectrum.json` (spectrum.report, assembly=True) with its stats.csv columns
    (spectrum.assembly_columns)."""
    dir: object
    k: int = 21
    every: int = 1
    sketch_size: object = None    # `--spectrum-sketch S`: also `DIR/<sample>.sketch.npy` and the json's "sketch" object

    def after(self, eng, text, offs, lens):
        """Per sample of a batch of FASTA text in HBM: (row, status), with a sketch size (row, status, the sketch's
        hashes, its eligible count).  A sample with a status has a zero row."""
        kw = {} if self.sketch_size is None else {"sketch": (self.sketch_size, 1)}
        rows, status, *rest = eng.spectrum_fasta(text, offs, lens, k=self.k, every=self.every, **kw)
        if self.sketch_size is None:
            return [(rows[j], int(status[j])) for j in range(len(rows))]
        hashes, info = rest
        return [(rows[j], int(status[j]), hashes[j, :int(info[j, 1])].copy(), int(info[j, 0])) for j in range(len(rows))]

    def emit(self, sample, got, stats_row, pool, writes):
        """A sample's file queued on the pool (its future goes to `writes`) and its columns into stats_row (None: none)."""
        from . import sketch, spectrum
        row, sk = got[0], None
        if self.sketch_size is not None:
            hashes, eligible = got[2], got[3]
            sk = sketch.meta(self.sketch_size, 1, eligible, len(hashes))
            writes.append(pool.submit(sketch.write_sketch, self.dir, sample, hashes))
        if stats_row is not None:
            stats_row.update(spectrum.assembly_columns(row, self.k, self.every))
        writes.append(pool.submit(spectrum.write_report, self.dir, sample, spectrum.report(row, self.k, self.every, sketch=sk,
                                                                                           assembly=True)))


def _seed_groups(names, seeds):
    """{seed: [indices into names]}: samples with different seeds go in separate calls."""
    by_seed = OrderedDict()
    for j, s in enumerate(names):
        by_seed.setdefault(int(seeds.get(s, 0)), []).append(j)
    return by_seed


def _ladders(eng, text, offs, lens, names, seeds, **ladder):
    """subsample.ladder_counts for the samples `names` in HBM (text[offs[i] .. +lens[i])), one launch per seed:
    samples with different seeds go in separate calls.  The records, in the samples' order."""
    from .subsample import ladder_counts
    recs = [None] * len(names)
    for seed, idx in _seed_groups(names, seeds).items():
        for j, r in zip(idx, ladder_counts(eng, text, offs[idx], lens[idx], seed=seed, **ladder)):
            recs[j] = r
    return recs


def _ladder_plans(eng, text, offs, lens, names, **ladder):
    """_ladders' records without the counting (a run that only writes step C's files): the read index and the plan;
    a step is (bp, None, None)."""
    from .subsample import ladder_plan
    nsites, status = eng.read_index(text, offs, lens)
    recs, plans = ladder_plan(nsites, status, **ladder)
    for rec, sizes in zip(recs, plans):
        rec["steps"] = [(bp, None, None) for bp in sizes]
    return recs


class SplitSink:
    """Where step C's files go: `<split_dir>/<sample>@<bp>K.fq.gz` (split_fastq, commands/image.py:696-714), gzip'ed on
    the pool like the cleaned reads of clean_dir.  A sample whose files are all there is left alone unless `overwrite`
    (:711-714); a file gets its name only once it is whole (written under a temporary name without the `@`, then renamed), so a run that
    was killed leaves nothing that the next one would take for done.  At most MAX_PENDING_BYTES of text wait for
    their gzip, besides the slice being queued.

    gpu_gzip: a slice's files are compressed where they lie in HBM (ImageEngine.deflate: BGZF), only the compressed
    bytes are copied back, and the pool job writes them as they are; MAX_PENDING_BYTES then counts compressed bytes."""

    MAX_PENDING_BYTES = 1 << 30

    def __init__(self, split_dir, pool, overwrite, gpu_gzip=False):
        self.dir, self.pool, self.overwrite, self.gpu_gzip = Path(split_dir), pool, overwrite, gpu_gzip
        self.pending = []   # [(the futures of one slice, its bytes on the host)], oldest first
        self.dir.mkdir(parents=True, exist_ok=True)

    def path(self, sample, bp):
        from .subsample import split_name
        return self.dir / (split_name(sample, bp) + ".fq.gz")

    def done(self, sample, sizes):
        return not self.overwrite and all(self.path(sample, bp).is_file() for bp in sizes)

    @staticmethod
    def _write(path, text, compressed=False):
        """text: the file's text, or with `compressed` the .gz file's own bytes"""
        import gzip
        part = path.with_name(".part." + path.name.replace(SAMPLE_BP_SEP, "+"))   # (no file of a sample to the default entry)
        with open(part, "wb") as fh:
            fh.write(text if compressed else gzip.compress(text, compresslevel=1))
        os.replace(part, path)

    def _drain(self, room):
        """Wait for the oldest slices' files until no more than `room` bytes of text are waiting."""
        while self.pending and sum(n for _, n in self.pending) > room:
            for fut in self.pending.pop(0)[0]:
                fut.result()

    def emit(self, eng, text, offs, lens, names, recs, seeds, **ladder):
        """The files of the samples `names` in HBM whose ladder `recs` (_ladders / _ladder_plans) has steps: emitted
        on the GPU by the counting's own plan (subsample.ladder_files), copied back a slice at a time, queued.  A sample
        that the emit's framing check refuses gets the error of a failed split in its record and loses its steps."""
        from .subsample import ladder_files
        for seed, idx in _seed_groups(names, seeds).items():
            skip = set()
            for local, j in enumerate(idx):
                sizes = [bp for bp, _, _ in recs[j]["steps"]]
                if sizes and self.done(names[j], sizes):
                    eprint("Skipping subsampling for", names[j] + ":", "Files exist.")
                    skip.add(local)
            nsites = [recs[j]["nsites"] for j in idx]
            status = [recs[j]["status"] for j in idx]
            failed = {}
            for dev, steps in ladder_files(eng, text, offs[idx], lens[idx], nsites, status, seed=seed, skip=skip,
                                           failed=failed, **ladder):
                self._drain(self.MAX_PENDING_BYTES)
                if self.gpu_gzip and steps:   # the slice's files compressed before they leave the device
                    gz, go, gl = eng.deflate(dev, [o for _, _, o, _ in steps], [n for _, _, _, n in steps])
                    host = gz[:int(go[-1] + gl[-1])].cpu().numpy()
                    del dev, gz
                    steps = [(local, bp, int(o), int(n)) for (local, bp, _, _), o, n in zip(steps, go, gl)]
                else:
                    host = dev.cpu().numpy()
                    del dev
                # (gzip reads a file's bytes where they lie in the slice: no second copy)
                self.pending.append(([self.pool.submit(self._write, self.path(names[idx[local]], bp), host[o:o + n], self.gpu_gzip)
                                      for local, bp, o, n in steps], host.nbytes))
            for local, st in failed.items():
                recs[idx[local]]["error"] = "inconsistent FASTQ framing (status %d writing the files)" % st
                recs[idx[local]]["steps"] = []

    def finish(self):
        """Wait for every file (a failed write raises here)."""
        self._drain(-1)


def _ladder_images(eng, text, offs, lens, names, sources, t0, sink, stats, seeds, splits=None, no_image=False, **ladder):
    """Steps C+D+E for one batch of cleaned samples in HBM (text[offs[i] .. +lens[i]) is sample names[i], read from
    sources[i]; the batch was begun at t0): the ladder (seeds by sample, **ladder: min_bp, max_bp, is_query), with
    `splits` (SplitSink) its files, the images, the stats rows and the PNG jobs (to `sink`); no_image: the ladder's plan
    and files only.  Returns the times the ladder and the images were done."""
    import torch

    from .subsample import split_name
    k = sink.k
    if no_image:
        recs = _ladder_plans(eng, text, offs, lens, names, **ladder)
    else:
        recs = _ladders(eng, text, offs, lens, names, seeds, **ladder)
    t_counted = time.perf_counter()
    if splits is not None:   # (the files are the splitting's time, not the counting's)
        splits.emit(eng, text, offs, lens, names, recs, seeds, **ladder)
    t1 = time.perf_counter()
    flat = [] if no_image else [(j, bp, h) for j, r in enumerate(recs) for bp, h, _ in r["steps"]]
    imgs = sink.rows(eng.images(torch.stack([h for _, _, h in flat]))) if flat else []
    nz = [bool((h != 0).any().item()) for _, _, h in flat]
    t2 = time.perf_counter()
    for j, s in enumerate(names):
        st = stats.setdefault(s, OrderedDict())
        if recs[j]["error"]:
            eprint("SPLIT FAIL:", sources[j], "-", recs[j]["error"])
            st["failed_step"] = "split"
            continue
        st["splitting_time"] = (t1 - t0) / len(names)
        st["splitting_bp_per_file"] = ",".join(str(bp) for bp, _, _ in recs[j]["steps"])
        if not no_image:
            st[str(k) + "mer_counting_time"] = (t_counted - t0) / len(names)
    for n, (j, bp, _) in enumerate(flat):
        s = names[j]
        if not nz[n]:
            eprint("IMAGE FAIL:", split_name(s, bp))
            stats[s]["failed_step"] = "image"
            continue
        sink.submit(s, s, png_name(split_name(s, bp) + "+k" + str(k) + ".fq.h5", sink.mapping_code), imgs[n])
    return t1, t2


def _sample_files(files):
    """A raw sample's files in the order step B reads them: (path, role) with single-end files first, then R1, then R2,
    each sorted (rawinput.pair_files; concatenate_reads, commands/image.py:264-315)."""
    from . import _capi
    from .rawinput import pair_files
    p = pair_files(files)
    return ([(f, _capi.VK_CL_ROLE_UNPAIRED) for f in sorted(p["unpaired"])] + [(f, _capi.VK_CL_ROLE_R1) for f in sorted(p["R1"])] +
            [(f, _capi.VK_CL_ROLE_R2) for f in sorted(p["R2"])])


def _budget(avgs, lines, sample_files, max_bp):
    """Records of each file (rawinput.reads_needed) for one sample: sample_files [(path, role)], its files' mean read
    lengths (0 without a read budget) and newline counts."""
    from . import _capi
    from .rawinput import reads_needed
    info = {"unpaired": [], "R1": [], "R2": []}
    key = {_capi.VK_CL_ROLE_UNPAIRED: "unpaired", _capi.VK_CL_ROLE_R1: "R1", _capi.VK_CL_ROLE_R2: "R2"}
    for j, (f, role) in enumerate(sample_files):
        info[key[role]].append({"file": f, "avg_length": avgs[j], "total_reads": int(lines[j]) // 4})
    take = reads_needed(info, max_bp)
    return [int(take.get(f, 0)) for f, _ in sample_files]


def _raw_plans(samples, weights, rank, world, bam=None):
    """This rank's share of raw samples [(sample, [files])] as [(sample, [(file, role)])], dealt by weight (per sample:
    the sum of its files' weights; None: agreed on here, a collective when sharded).  bam (the options of `--from-bam`):
    a sample is one BAM file and its plan [(file, role, select)] (bam.sample_plan).  With bam["groups"] ({sample: its
    group's index in its file}: `--bam-read-groups`) the samples of one file make ONE plan [(file, role, select, group,
    sample)] under the file's name: a file is uploaded once for all of its groups, so they stay in one batch and on one
    rank."""
    if bam is not None and bam.get("groups") is not None:
        from .bam import sample_plan
        units, at = OrderedDict(), {}
        for i, (s, files) in enumerate(samples):
            units.setdefault(files[0], []).append(s)
            at.setdefault(files[0], i)
        plans = [(str(f), [e + (s,) for s in members for e in sample_plan(f, bam.get("pairs", False), bam["groups"][s])])
                 for f, members in units.items()]
        if weights is not None:   # (one per sample, each its file's: a unit weighs what its file weighs)
            weights = [weights[at[f]] for f in units]
    elif bam is not None:
        from .bam import sample_plan
        plans = [(s, sample_plan(files[0], bam.get("pairs", False))) for s, files in samples]
    else:
        plans = [(s, _sample_files(files)) for s, files in samples]
    if weights is None:
        weights = sample_weights([(s, list(dict.fromkeys(e[0] for e in sf))) for s, sf in plans], world)
    return [plans[i] for i in shard_by_size(weights, rank, world)]


@dataclass
class Cleaning:
    """Step B's options as raw_to_images and raw_to_query take them (their docstrings)."""
    trim: tuple
    adapter: bool
    merge: bool
    dedup: bool
    adapters: tuple
    detect_adapters: bool
    clean_dir: object
    max_bp: int
    gpu_gzip: bool = False
    screen: object = None   # `--exclude-fasta` / `--keep-fasta`: a Screen, applied right after the cleaning
    qc: object = None   # `--qc-report`: a QcReport
    spectrum: object = None   # `--kmer-spectrum`: a Spectrum
    bam: object = None   # `--from-bam`: {"pairs": bool, "exclude": int, "groups": None or {sample: group}}; the plans then hold (file, role, select[, group, sample])


def _bam_texts(eng, batch, pool, bam):
    """`--from-bam`'s step between the upload and the cleaning, for a batch [(sample, [(file, role, select)])]: the
    files' headers are read on the host (bam.bam_header), their bytes uploaded and inflated in HBM
    (ImageEngine.upload_files), converted to one FASTQ text per (file, role) there (ImageEngine.bam_to_fastq) and
    released.  Returns (text, offsets, lengths, {index in the batch: why it failed}): a file that is not BAM, whose
    header does not parse or whose records give a status fails its sample; its texts are empty.

    With bam["groups"] (`--bam-read-groups`) the batch is [(file, [(file, role, select, group, sample)])] and a text is
    made per (file, role, group) (ImageEngine.bam_groups_frame / bam_groups_fastq): the file is uploaded and inflated once
    for all of its groups.  The reads of no listed group are counted by streams of their own, reported per file and not
    written."""
    from .bam import BamError, file_info, read_groups
    grouped = bam.get("groups") is not None
    files = list(dict.fromkeys(Path(e[0]) for _, plan in batch for e in plan))
    heads, why, ids = {}, {}, {}
    for f in files:
        try:
            heads[f] = file_info(f)[1]   # (read when the batch was sized: not again)
            if grouped:
                ids[f] = read_groups(f)
        except (BamError, OSError) as e:
            heads.pop(f, None)
            why[f] = str(e) or type(e).__name__
    good = [f for f in files if f in heads]
    at = {f: i for i, f in enumerate(good)}
    streams = [(j, Path(e[0]), e[2]) + ((e[3],) if grouped else ()) for j, (_, plan) in enumerate(batch) for e in plan]
    offs = np.zeros(len(streams), dtype=np.uint64)
    lens = np.zeros(len(streams), dtype=np.uint64)
    text, failed = None, {}
    if good:
        dev, doffs, dlens = eng.upload_files(good, pool)
        live = [i for i, st in enumerate(streams) if st[1] in at]
        first, n_ref = [heads[f][0] for f in good], [heads[f][1] for f in good]
        exclude = bam.get("exclude", 0x900)
        if grouped:
            text, oo, ol, status = _bam_group_texts(eng, dev, doffs, dlens, first, n_ref, [ids[f] for f in good], good,
                                                    [(at[streams[i][1]], streams[i][2], streams[i][3]) for i in live],
                                                    bam.get("pairs", False), exclude)
        else:
            text, oo, ol, status = eng.bam_to_fastq(dev, doffs, dlens, first, n_ref, [at[streams[i][1]] for i in live],
                                                    [streams[i][2] for i in live], exclude=exclude)
        del dev
        offs[live], lens[live] = oo, ol
        inflate = getattr(eng, "last_upload_status", None)   # (a member that does not inflate or fails its CRC: no bytes)
        for f in good:
            if inflate is not None and inflate[at[f]]:
                why[f] = "inflate status %d" % int(inflate[at[f]])
            elif status[at[f]]:
                why[f] = "BAM status %d" % int(status[at[f]])
    for j, f, *_ in streams:
        if f in why:
            failed[j] = why[f]
    return text, offs, lens, failed


def _bam_group_texts(eng, dev, doffs, dlens, first, n_ref, groups, files, streams, pairs, exclude):
    """The texts of the streams [(file index, select, group)] of files in HBM, split by read group: one framing call that
    also counts, per file, the reads of no listed group (streams of VK_BAM_UNGROUPED, reported on stderr and not
    written), then one text call for the streams that have reads.  Returns (text, offsets, lengths, status) as
    ImageEngine.bam_to_fastq does: a stream without reads has no bytes."""
    from . import _capi
    selects = (_capi.VK_BAM_SINGLE, _capi.VK_BAM_READ1, _capi.VK_BAM_READ2) if pairs else (_capi.VK_BAM_ALL,)
    loose = [(i, sel, _capi.VK_BAM_UNGROUPED) for i in range(len(files)) for sel in selects]
    every = list(streams) + loose
    recs, nbytes, status = eng.bam_groups_frame(dev, doffs, dlens, first, n_ref, groups, [s[0] for s in every],
                                                [s[1] for s in every], [s[2] for s in every], exclude=exclude)
    passed = np.zeros(len(files), dtype=np.int64)
    for (i, _, _), n in zip(loose, recs[len(streams):]):
        passed[i] += int(n)
    for i, f in enumerate(files):
        if passed[i] and not status[i]:
            eprint(f"{f}: {int(passed[i])} reads without a listed read group passed over")
    oo = np.zeros(len(streams), dtype=np.uint64)
    ol = np.zeros(len(streams), dtype=np.uint64)
    full = [k for k in range(len(streams)) if nbytes[k]]
    text = None
    if full:
        from .engine import slots16
        oo[full], pos = slots16(nbytes[full])
        import torch
        text = torch.zeros(pos + 16, dtype=torch.uint8, device=eng.device)
        got, status = eng.bam_groups_fastq(dev, doffs, dlens, first, n_ref, groups, [streams[k][0] for k in full],
                                           [streams[k][1] for k in full], [streams[k][2] for k in full], text, oo[full],
                                           nbytes[full], exclude=exclude)
        ol[full] = got
    return text, oo, ol, status


def _clean_batches(eng, mine, pool, writes, stats, base_sd, opt, batch_bytes, verbose):
    """Step B for this rank's raw samples `mine` [(sample, [(file, role)])] under the options `opt` (Cleaning), as
    raw_to_images and raw_to_query share it: batch after batch is uploaded (a .gz inflated in HBM), gets its read
    budget (the files' line counts and mean read lengths, one call each for the batch: ImageEngine.clean_lines /
    clean_heads), its adapters and is cleaned.
    Yields (text on the device, offsets, lengths, samples, time the cleaning was done) for the samples of a batch that
    came through; the others are reported (CLEAN FAIL) and get `failed_step` in stats.  Fills stats (`clean_basepairs`,
    `cleaning_time`) and base_sd, and with opt.clean_dir queues the writes of `<sample>.fq.gz` and
    `<sample>_fastp_gpu.json` on the pool (their futures go to `writes`)."""
    import gzip
    import json

    from .rawinput import content_curves, curves_sd
    by_sequence = opt.adapters is not None or opt.detect_adapters
    if by_sequence and not opt.adapter:
        raise ValueError("adapters by sequence need adapter trimming (not -a)")
    explicit = [None, None, None]
    if opt.adapters is not None:
        a1, a2 = opt.adapters
        explicit = [a1, a2 if a2 is not None else a1, a1]
    clean_dir = None if opt.clean_dir is None else Path(opt.clean_dir)
    if clean_dir is not None:
        clean_dir.mkdir(parents=True, exist_ok=True)

    def write_clean(sample, text, curves, cutting=None, compressed=False, screened=None):
        """text: the cleaned reads, or with `compressed` the .fq.gz file's own bytes (opt.gpu_gzip)"""
        with open(clean_dir / (sample + ".fq.gz"), "wb") as fh:
            fh.write(text if compressed else gzip.compress(text, compresslevel=1))
        report = {"read1_after_filtering": {"content_curves": curves}}
        if cutting is not None:
            report["adapter_cutting"] = cutting
        if screened is not None:
            report["screen"] = screened
        with open(clean_dir / (sample + "_fastp_gpu.json"), "w") as fh:
            json.dump(report, fh)

    if opt.bam is not None:
        from .bam import batch_bytes as bam_bytes

        def size(plan):
            return sum(bam_bytes(f) for f in dict.fromkeys(e[0] for e in plan[1]))
    else:
        def size(plan):
            return sum(text_bytes(f) for f, _ in plan[1])

    for batch, nbytes, t0 in batches(mine, batch_bytes, size=size):
        if opt.bam is not None:   # BAM bytes in, one FASTQ text per (file, role) out; from here on the run is --from-raw's
            dev, offs, lens, bad = _bam_texts(eng, batch, pool, opt.bam)
            grouped = opt.bam.get("groups") is not None
            for j, why in bad.items():
                eprint("CLEAN FAIL:", sorted({str(e[0]) for e in batch[j][1]}), "-", why)
                for s in (dict.fromkeys(e[4] for e in batch[j][1]) if grouped else [batch[j][0]]):
                    stats.setdefault(s, OrderedDict())["failed_step"] = "clean"
            nstreams = [len(plan) for _, plan in batch]
            first = np.concatenate(([0], np.cumsum(nstreams)))
            keep = [j for j in range(len(batch)) if j not in bad]
            # A stream without reads (--bam-pairs on a file of mates only, or of single reads only) is no file of the
            # sample, as a role without files is none of a raw sample's; a sample without any read keeps one empty
            # stream and fails where a raw sample of an empty file fails.  A stream per role of ONE file: named
            # apart, the read budget is kept by name.
            # `--bam-read-groups`: a file's plan holds the streams of all of its groups; each group with reads is a
            # sample of its own from here on, and a group without reads is none.
            rows, plans = [], []
            for j in keep:
                members = OrderedDict()
                for i in range(first[j], first[j + 1]):
                    members.setdefault(batch[j][1][i - first[j]][4] if grouped else batch[j][0], []).append(i)
                for s, own in members.items():
                    mine = [i for i in own if lens[i]] or ([] if grouped else [own[0]])
                    if not mine:
                        if verbose:
                            eprint(f"{batch[j][0]}: read group sample {s} has no reads: no sample")
                        continue
                    rows += mine
                    plans.append((s, [(f"{e[0]}:{('single', 'R1', 'R2')[e[1]]}" + (f":{e[3]}" if grouped else ""), e[1])
                                      for e in (batch[j][1][i - first[j]] for i in mine)]))
            offs, lens, batch = offs[rows], lens[rows], plans
            if not batch:
                continue
        else:
            paths = [Path(f) for _, sf in batch for f, _ in sf]
            dev, offs, lens = eng.upload_files(paths, pool)
        lines = eng.clean_lines(dev, offs, lens)
        avgs = [0] * len(lines)
        if opt.max_bp is not None:   # (the mean length of each file's first 10,000 reads: estimate_read_lengths, commands/image.py:90-115)
            totals, counted = eng.clean_heads(dev, offs, lens, 10000)
            avgs = [round(int(t) / int(n)) if n else 0 for t, n in zip(totals, counted)]
        records, roles, owner, failed = [], [], [], set()
        at = 0
        for j, (s, sf) in enumerate(batch):
            sl = slice(at, at + len(sf))
            try:
                records += _budget(avgs[sl], lines[sl], sf, opt.max_bp)
            except ZeroDivisionError:     # (a file without reads and a read budget: the reference fails here too)
                records += [0] * len(sf)
                failed.add(j)
            roles += [r for _, r in sf]
            owner += [j] * len(sf)
            at += len(sf)
        table = None
        if by_sequence:
            found = (eng.detect_adapters(dev, offs, lens, records, roles, owner, len(batch), trim_tail=opt.trim[1])
                     if opt.detect_adapters else [[None] * 3 for _ in batch])
            table = [[e if e is not None else d for e, d in zip(explicit, det)] for det in found]
        out, ooffs, olens, cst, status, *rest = eng.clean(dev, offs, lens, records, roles, owner, len(batch), trim=opt.trim,
                                                          adapter=opt.adapter, merge=opt.merge, dedup=opt.dedup,
                                                          adapters=table)
        ast = rest[0] if rest else None   # (adapter stats: with a table only)
        qc_before = opt.qc.before(eng, dev, offs, lens, records, roles, owner, len(batch)) if opt.qc is not None else None
        del dev
        srows = None
        if opt.screen is not None:   # the cleaned text screened where it lies: the files and the ladder see what is kept
            out, ooffs, olens, srows = opt.screen.apply(eng, out, ooffs, olens, [s for s, _ in batch], None, pool)
        spec_rows = {}
        if opt.spectrum is not None:   # (behind the screen, once per sample: what the ladder sees)
            good = [j for j in range(len(batch)) if not status[j] and j not in failed]
            got = opt.spectrum.after(eng, out, ooffs[good], olens[good])
            if opt.spectrum.band is not None:   # `--depth-filter`: the files, the qc and the ladder see what is kept
                got, out, goffs, glens = got
                ooffs, olens = np.zeros_like(ooffs), np.zeros_like(olens)   # (a sample that failed is not looked at again)
                ooffs[good], olens[good] = goffs, glens
            spec_rows = dict(zip(good, got))
        qc_after = {}
        if opt.qc is not None:   # (behind the screen and the depth filter: what the ladder sees)
            good = [j for j in range(len(batch)) if not status[j] and j not in failed]
            qc_after = dict(zip(good, opt.qc.after(eng, out, ooffs[good], olens[good])))
        packed = {}
        if clean_dir is not None and opt.gpu_gzip:   # the cleaned text compressed where it lies: only the files' bytes come back
            good = [j for j in range(len(batch)) if not status[j] and j not in failed]
            if good:
                gz, go, gl = eng.deflate(out, ooffs[good], olens[good])
                host = gz[:int(go[-1] + gl[-1])].cpu().numpy()
                del gz
                packed = {j: host[int(o):int(o + n)] for j, o, n in zip(good, go, gl)}
        tc = time.perf_counter()
        ok = []
        for j, (s, sf) in enumerate(batch):
            st = stats.setdefault(s, OrderedDict())
            if status[j] or j in failed:
                eprint("CLEAN FAIL:", [f for f, _ in sf], "- status", int(status[j]))
                st["failed_step"] = "clean"
                continue
            row = cst[j]
            curves = content_curves(row[2:2 + 160], row[162:202])
            base_sd[s] = curves_sd(curves)
            st["clean_basepairs"] = int(row[0]) if (opt.adapter or opt.merge) else float("nan")
            st["cleaning_time"] = (tc - t0) / len(batch)
            if srows is not None:
                st.update(opt.screen.columns(srows[j]))
            if opt.qc is not None:
                opt.qc.emit(s, qc_before[j], qc_after[j], st, pool, writes)
            if opt.spectrum is not None:
                opt.spectrum.emit(s, spec_rows[j], st, pool, writes)
            if clean_dir is not None:
                text = packed[j] if opt.gpu_gzip else out[int(ooffs[j]):int(ooffs[j]) + int(olens[j])].cpu().numpy().tobytes()
                cutting = None
                if by_sequence:
                    name = [a.decode("latin-1") if a is not None else None for a in table[j]]
                    cutting = {"read1_adapter_sequence": name[0], "read2_adapter_sequence": name[1],
                               "single_adapter_sequence": name[2], "adapter_trimmed_reads": int(ast[j][0]),
                               "adapter_trimmed_bases": int(ast[j][1])}
                screened = None if srows is None else opt.screen.report(opt.screen.set_on(eng), srows[j])
                writes.append(pool.submit(write_clean, s, text, curves, cutting, opt.gpu_gzip, screened))
            ok.append(j)
        if verbose:
            eprint(f"batch of {len(batch)} samples, {nbytes} raw bytes: upload+clean {tc - t0:.3f}s")
        if ok:
            yield out, ooffs[ok], olens[ok], [batch[j][0] for j in ok], tc


def raw_to_images(samples, outdir, k=7, mapping_code="cgr", min_bp=50000, max_bp=None, trim=(10, 10), adapter=True,
                  merge=True, dedup=True, seeds=None, labels=None, subfolder_levels=0, device=0, rank=0, world=1,
                  batch_bytes=None, io_threads=8, engine=None, verbose=False, weights=None, clean_dir=None, adapters=None,
                  detect_adapters=False, split_dir=None, overwrite=False, no_image=False, gpu_gzip=False, bam=None,
                  gpu_png=False, screen=None, qc_dir=None, spectrum=None):
    """Steps B+C+D+E of run_clean2img (commands/image.py:938-1127) for RAW reads: samples = [(sample, [files])] as
    rawinput.process_input lists them.  A batch of samples is uploaded (a .gz inflated in HBM), cleaned on the GPU
    (ImageEngine.clean: vk_clean_device) and the cleaned text goes straight to the ladder of clean_to_images, without
    leaving the device.  clean_dir: also write `<sample>.fq.gz` and `<sample>_fastp_gpu.json` (the content curves
    get_basefrequency_sd reads) there, as the reference's intermediate folder holds them.

    adapters = (R1 and single reads' sequence, R2's sequence or None: the first) and detect_adapters: also trim by
    sequence ("Step B"); an explicit sequence wins over detection for its groups, detection runs per
    batch (ImageEngine.detect_adapters) after the read budget.  The JSON then holds `adapter_cutting`.

    split_dir, overwrite, no_image: as clean_to_images takes them.  gpu_gzip: the .fq.gz files of clean_dir and split_dir
    are compressed on the GPU (ImageEngine.deflate: BGZF) and only their bytes are copied back.  gpu_png: the images' IDAT chunks are made on the GPU (PngSink).

    bam = {"pairs": bool, "exclude": int}: `--from-bam` -- every sample is ONE BAM file, converted to FASTQ text in HBM
    between the upload and the cleaning (_bam_texts; the rule: INTEGRATION.md, "--from-bam: the rule").

    screen (Screen): `--exclude-fasta` / `--keep-fasta` -- the cleaned text is screened in HBM right after the cleaning,
    so clean_dir's files, split_dir's files and the ladder see the reads that are kept; the stats gain `screen_reads_in`,
    `screen_reads_removed`, `screen_basepairs_removed` (`clean_basepairs` and the base-frequency sd stay the cleaning's).

    qc_dir: `--qc-report` -- `<qc_dir>/<sample>.qc.json` (QcReport) of the raw texts under their read budget and of the
    cleaned text behind the screen; the stats gain qc.columns' columns.

    spectrum (Spectrum): `--kmer-spectrum` -- `<dir>/<sample>.spectrum.json` of the cleaned text behind the screen, counted
    once per sample (never per ladder step); the stats gain spectrum.columns' columns.

    Returns ({sample: OrderedDict(stats)}, {sample: base-frequency sd}) with the reference's keys `clean_basepairs`
    (nan with neither adapter trimming nor merging, commands/image.py:551-565), `cleaning_time`, then those of
    clean_to_images, or `failed_step`."""
    mine = _raw_plans(samples, weights, rank, world, bam)
    opt = Cleaning(trim, adapter, merge, dedup, adapters, detect_adapters, clean_dir, max_bp, gpu_gzip, screen,
                   None if qc_dir is None else QcReport(qc_dir), spectrum, bam)
    stats, base_sd, writes = OrderedDict(), {}, []
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        sink = PngSink(outdir, pool, k, mapping_code, labels or {}, base_sd, subfolder_levels, eng if gpu_png else None)
        splits = SplitSink(split_dir, pool, overwrite, gpu_gzip) if split_dir is not None else None
        for out, ooffs, olens, names, tc in _clean_batches(eng, mine, pool, writes, stats, base_sd, opt,
                                                           batch_bytes or DEFAULT_BATCH_BYTES, verbose):
            _ladder_images(eng, out, ooffs, olens, names, names, tc, sink, stats, seeds or {}, splits=splits,
                           no_image=no_image, min_bp=min_bp, max_bp=max_bp, is_query=False)
        for w in writes:
            w.result()
        if splits is not None:
            splits.finish()
        sink.finish(stats)
    return stats, base_sd


def _query_rungs(eng, text, offs, lens, names, sources, seeds, max_bp, base_sd, found):
    """Step C of a query for cleaned samples in HBM: the one subsample that `query` images (split_fastq with
    is_query, commands/image.py:677-701).  found[sample] = (bp, histogram on the device, sd); a sample without one
    is reported (SPLIT FAIL) and left out."""
    for s, source, rec in zip(names, sources, _ladders(eng, text, offs, lens, names, seeds, max_bp=max_bp, is_query=True)):
        if rec["error"] or not rec["steps"]:
            eprint("SPLIT FAIL:", source, "-", rec["error"])
            continue
        bp, hist, _ = rec["steps"][0]
        found[s] = (bp, hist, base_sd.get(s, 0))


def raw_to_query(samples, k=7, mapping_code="cgr", max_bp=None, trim=(10, 10), adapter=True, merge=True, dedup=True,
                 seeds=None, device=0, rank=0, world=1, batch_bytes=None, io_threads=8, engine=None, verbose=False,
                 weights=None, clean_dir=None, adapters=None, detect_adapters=False, gpu_gzip=False, bam=None, screen=None,
                 qc_dir=None, spectrum=None):
    """Steps B+C of run_clean2img as `varKoder query` runs it (commands/query.py:97-178): raw_to_images' batches, each
    cleaned sample subsampled once (-M) and counted.  Returns {sample: (bp, histogram uint32[4^k] on the device,
    base-frequency sd)} for this rank's samples in the order they were dealt; one that fails in clean or split is
    reported (CLEAN FAIL / SPLIT FAIL) and left out, the others go on.  Nothing is written except, with clean_dir,
    the cleaned reads and their reports as raw_to_images writes them (gpu_gzip: compressed on the GPU), and with qc_dir
    the samples' `.qc.json`, with spectrum their `.spectrum.json`.  bam, screen, qc_dir, spectrum: as raw_to_images takes them."""
    mine = _raw_plans(samples, weights, rank, world, bam)
    opt = Cleaning(trim, adapter, merge, dedup, adapters, detect_adapters, clean_dir, max_bp, gpu_gzip, screen,
                   None if qc_dir is None else QcReport(qc_dir), spectrum, bam)
    stats, base_sd, found, writes = OrderedDict(), {}, OrderedDict(), []
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        for out, ooffs, olens, names, _ in _clean_batches(eng, mine, pool, writes, stats, base_sd, opt,
                                                          batch_bytes or DEFAULT_BATCH_BYTES, verbose):
            _query_rungs(eng, out, ooffs, olens, names, names, seeds or {}, max_bp, base_sd, found)
        for w in writes:
            w.result()
    return found


def clean_to_query(samples, base_sd=None, max_bp=None, seeds=None, engine=None, k=7, mapping_code="cgr", device=0,
                   batch_bytes=None, io_threads=8, screen=None, qc_dir=None, spectrum=None):
    """raw_to_query's result for samples = [(sample, its cleaned read file)] that an earlier run left in clean_dir
    (this rank's share, the files as they are; base_sd: their figures, image.base_sd_table).  screen (Screen): the
    uploaded reads are screened in HBM before they are subsampled.  qc_dir (`--qc-report`): `<qc_dir>/<sample>.qc.json`
    of the uploaded reads (behind the screen), its `after` sections only.  spectrum (Spectrum, `--kmer-spectrum`):
    `<dir>/<sample>.spectrum.json` of the uploaded reads (behind the screen)."""
    samples = [(s, Path(f)) for s, f in samples]
    found, reports = OrderedDict(), []
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        for batch, _, _ in batches(samples, batch_bytes or DEFAULT_BATCH_BYTES, size=lambda sample: text_bytes(sample[1])):
            files = [f for _, f in batch]
            dev, offs, lens = eng.upload_files(files, pool)
            if screen is not None:
                dev, offs, lens, _ = screen.apply(eng, dev, offs, lens, [s for s, _ in batch], None, pool)
            spec_rows = None
            if spectrum is not None:   # (before the qc: with `--depth-filter` the qc and the rung see what is kept)
                spec_rows = spectrum.after(eng, dev, offs, lens)
                if spectrum.band is not None:
                    spec_rows, dev, offs, lens = spec_rows
            if qc_dir is not None:
                for (s, _), row in zip(batch, QcReport.after(eng, dev, offs, lens)):
                    QcReport(qc_dir).emit(s, None, row, None, pool, reports)
            if spectrum is not None:
                for (s, _), row in zip(batch, spec_rows):
                    spectrum.emit(s, row, None, pool, reports)
            _query_rungs(eng, dev, offs, lens, [s for s, _ in batch], files, seeds or {}, max_bp, base_sd or {}, found)
        for w in reports:
            w.result()
    return found
