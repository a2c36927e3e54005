"""`image --from-fasta` / `query --from-fasta`: assemblies, contigs, organelle genomes -- FASTA files, one sample per
file, counted whole on the GPU (ImageEngine.count_fasta; the rule: INTEGRATION.md, "--from-fasta") and imaged like any
histogram.  Stands where the reference would hand dsk a FASTA `-file` (commands/image.py:771-796).

`image --from-fasta --fragments` draws the 1-2-5 subsample ladder of the read entries from an assembly (the rule:
INTEGRATION.md, "--from-fasta --fragments"): the joined bases of a sample are tiled into fragments of `--fragment-length`
bases, shifted per step; a step of `bp` bases takes each fragment with probability bp / bases (sample_hash of the step's
seed and the fragment's number) and counts the k-mers inside the taken fragments (ImageEngine.count_fasta_sampled).
fasta_plan is the plan (names, seeds, thresholds, shifts: host arithmetic), fasta_ladder runs it on a batch in HBM, and
fasta_to_images(fragments=True) images every step as `<sample>@<bp>K+<mapping>+k<k>.png`, bp the step's size.

`image / query --from-fasta --per-record` make every record of a file a sample of its own (the rule: INTEGRATION.md,
"--from-fasta --per-record"): ImageEngine.fasta_records gives the record table of a batch, record_names the samples'
names, record_plan the calls of ImageEngine.count_fasta_records, a row per selected record.

`image / query --from-fasta --windows` make every window of `--window-length` bases of a record, one every
`--window-step` bases, a sample of its own (the rule: INTEGRATION.md, "--from-fasta --windows"): window_counts gives the
windows of every record, window_names their sample names, window_plan the first row of every record and the row ranges
of the ImageEngine.count_fasta_windows calls."""
import re
import time
from collections import OrderedDict
from pathlib import Path

import numpy as np

from .image import eprint
from .pipeline import DEFAULT_BATCH_BYTES, PngSink, _seed_groups, batches, engine_scope, text_bytes
from .shard import agreed_weights, file_weights, shard_by_size
from .subsample import ladder_plan, plan_steps, split_name

FASTA_SUFFIXES = (".fa", ".fasta", ".fna")


def sample_of(path):
    """The sample a FASTA file holds: its name up to the suffix (.fa, .fasta, .fna, each also .gz); None: not one."""
    name = Path(path).name
    if name.endswith(".gz"):
        name = name[:-3]
    for suffix in FASTA_SUFFIXES:
        if name.endswith(suffix) and len(name) > len(suffix):
            return name[:-len(suffix)]
    return None


def fasta_files(src):
    """The FASTA files of folder `src`, sorted by name; two files of one sample are an error."""
    files = sorted(f for f in Path(src).iterdir() if f.is_file() and sample_of(f) is not None)
    seen = {}
    for f in files:
        s = sample_of(f)
        if s in seen:
            raise Exception(f"Two FASTA files for sample {s}: {seen[s].name} and {f.name}")
        seen[s] = f
    return files


def image_name(sample, bases, k, mapping_code):
    """`<sample>@<bp>K+<mapping>+k<k>.png`, bp = the sample's sequence bytes."""
    return split_name(sample, bases) + f"+{mapping_code}+k{k}.png"


def sample_hash(seed, anchor):
    """csrc/vk_lane.h's sample_hash: what decides whether a step takes a fragment (anchor: the fragment's number)."""
    m = 0xFFFFFFFF
    h = (anchor ^ seed) & m
    h = (h + ((anchor >> 32) * 0x9E3779B1 & m) + (seed >> 32)) & m
    h ^= h >> 16
    h = h * 0x85EBCA6B & m
    h ^= h >> 13
    h = h * 0xC2B2AE35 & m
    h ^= h >> 16
    return h


SAMPLED_HIST_BYTES = 1 << 30   # histograms of one count_fasta_sampled call


def fasta_plan(bases, status, frag_len, seed=0, min_bp=50000, max_bp=None):
    """The ladder of a batch of FASTA samples from their sequence bytes and status words: (records, steps) -- the records
    of subsample.ladder_plan over nsites = bases, and per step (sample, level, bp, seed + level, threshold, shift, whole)
    in the samples' order, largest first: subsample.plan_steps' tuples with the step's shift, sample_hash(its seed,
    2^64 - 1) mod frag_len, before `whole` (the step is the sample's plain count)."""
    recs, plans = ladder_plan(bases, status, min_bp, max_bp)
    for rec in recs:
        if rec["status"]:
            rec["error"] = "not a FASTA text"
    steps = [(i, level, bp, sd, thr, sample_hash(sd & (2 ** 64 - 1), 2 ** 64 - 1) % frag_len, whole)
             for i, level, bp, sd, thr, whole in plan_steps(plans, [int(b) for b in bases], seed)]
    return recs, steps


def fasta_ladder(engine, dev, offs, lens, frag_len, seed=0, min_bp=50000, max_bp=None):
    """All ladder steps of a batch of FASTA samples resident in HBM.  Returns one record per sample, shaped like
    subsample.ladder_counts' records: OrderedDict(nsites = its bases, status, steps=[(bp, hist uint32 tensor [4^k] on the
    device, bases taken)], error).  The step that holds all of a sample is its plain count (count_fasta); every other
    step of the batch goes into one count_fasta_sampled call (more when their histograms pass SAMPLED_HIST_BYTES)."""
    offs, lens = np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint64)
    hist, status, bases = engine.count_fasta(dev, offs, lens)
    bases_h = bases.cpu().numpy()
    recs, steps = fasta_plan(bases_h, status.cpu().numpy(), frag_len, seed, min_bp, max_bp)
    sampled = [st for st in steps if not st[6]]
    got = {}
    chunk = max(1, SAMPLED_HIST_BYTES // (4 * engine.ncode))
    for at in range(0, len(sampled), chunk):
        part = sampled[at:at + chunk]
        h, _, _, taken = engine.count_fasta_sampled(dev, offs, lens, frag_len, [st[0] for st in part],
                                                    [st[3] & (2 ** 64 - 1) for st in part], [st[4] for st in part],
                                                    [st[5] for st in part])
        taken = taken.cpu().numpy()
        for j, st in enumerate(part):
            got[st[:2]] = (h[j], int(taken[j]))
    for i, level, bp, *_, whole in steps:
        recs[i]["steps"].append((bp, hist[i], int(bases_h[i])) if whole else (bp,) + got[(i, level)])
    return recs


RECORD_HIST_BYTES = 1 << 30    # histograms of one count_fasta_records call
RECORD_ID_BYTES = 100


def record_names(file_sample, names):
    """The sample names of a file's records from their header lines (the bytes behind the '>'): (sample names, indices of
    the duplicates).  The id is the name up to the first blank, tab or \\r, every byte outside [A-Za-z0-9._-] replaced by
    '_', cut to RECORD_ID_BYTES, `record<ordinal + 1>` when empty; the sample name is `<file sample>__<id>`.  A later
    record whose sample name equals an earlier one's is a duplicate: the first stands."""
    out, dup, seen = [], [], set()
    for i, raw in enumerate(names):
        rid = bytes(raw)
        for sep in (b" ", b"\t", b"\r"):
            rid = rid.split(sep, 1)[0]
        rid = "".join(chr(b) if (48 <= b <= 57 or 65 <= b <= 90 or 97 <= b <= 122 or b in b"._-") else "_"
                      for b in rid[:RECORD_ID_BYTES])
        name = f"{file_sample}__{rid or 'record%d' % (i + 1)}"
        if name in seen:
            dup.append(i)
        seen.add(name)
        out.append(name)
    return out, dup


def record_plan(bases, min_len, hist_bytes=RECORD_HIST_BYTES, ncode=4 ** 7):
    """The count_fasta_records calls of a batch: the records with bases >= min_len (indices into `bases`, the batch's
    record table), in order, in runs whose rows (4 * ncode bytes each) fit in hist_bytes; a single row always fits."""
    per_call = max(1, int(hist_bytes) // (4 * int(ncode)))
    chosen = [i for i, b in enumerate(bases) if int(b) >= min_len]
    return [chosen[at:at + per_call] for at in range(0, len(chosen), per_call)]


WINDOW_HIST_BYTES = 1 << 30    # histograms of one count_fasta_windows call, tile rows included
NO_WINDOW = 0xFFFFFFFFFFFFFFFF  # VK_FA_NO_WINDOW
MAX_WINDOW_STEPS = 64           # window length / window step
_WINDOW_NAME = re.compile(r"(.+)__[0-9]+-[0-9]+$")


def window_limits(n, s, k):
    """Why (n, s) is no window length and step for k-mers of k bases (a sentence), or None: 100 <= n < 2^31 for the
    command line, k <= s <= n, s | n, n / s <= 64 (vk_count_fasta_windows_device's conditions)."""
    if not 100 <= n < 2 ** 31:
        return "the window length must be at least 100 and below 2^31"
    if not k <= s <= n:
        return f"the window step must lie between k = {k} and the window length"
    if n % s:
        return "the window length must be a multiple of the window step"
    if n // s > MAX_WINDOW_STEPS:
        return f"the window length must be at most {MAX_WINDOW_STEPS} window steps"
    return None


def window_counts(bases, n, s):
    """The windows of records of `bases` joined bytes: window w covers [w * s, w * s + n) and exists iff it lies within
    the record; no partial windows (int64 array; a negative entry, a passed-over record, has none)."""
    b = np.asarray(bases).astype(np.int64)
    return np.where(b >= n, (b - n) // s + 1, 0)


def window_name(record_sample, n, s, w):
    """`<record sample>__<start>-<end>` of a record's window w: 1-based, inclusive, decimal."""
    return f"{record_sample}__{w * s + 1}-{w * s + n}"


def window_names(record_sample, n, s, nwin):
    return [window_name(record_sample, n, s, w) for w in range(int(nwin))]


def window_plan(bases, n, s, hist_bytes=WINDOW_HIST_BYTES, ncode=4 ** 7):
    """The count_fasta_windows calls of a batch: (win_first, ranges).  Every record with bases >= n (indices into
    `bases`, the batch's record table; -1 marks a record to pass over, a duplicate) gets consecutive rows, one per
    window, from win_first[g] on (uint64; NO_WINDOW for the others).  ranges = [(row_lo, nrows, tile_rows)] cuts the
    rows into consecutive ranges whose histograms (4 * ncode bytes a row) fit in hist_bytes; with s < n that includes
    the tile rows a range needs: per record with a row in it, its rows there + n / s - 1 (0 when s == n).  A range may
    begin and end inside a record; a single row always fits."""
    m = n // s
    counts = window_counts(bases, n, s)
    win_first = np.full(len(counts), NO_WINDOW, dtype=np.uint64)
    ends = np.cumsum(counts)
    win_first[counts > 0] = (ends - counts)[counts > 0].astype(np.uint64)
    budget = max(1, int(hist_bytes) // (4 * int(ncode)))
    ranges, lo, nrows, tiles = [], 0, 0, 0
    for c in counts[counts > 0]:
        left = int(c)
        while left:
            room = budget - nrows - tiles
            fit = room if m == 1 else (room - (m - 1)) // 2   # a row of a record new to the range: itself, its tile, m - 1 more
            if fit <= 0 and nrows:
                ranges.append((lo, nrows, tiles))
                lo, nrows, tiles = lo + nrows, 0, 0
                continue
            take = min(left, max(fit, 1))
            nrows += take
            tiles += take + m - 1 if m > 1 else 0
            left -= take
    if nrows:
        ranges.append((lo, nrows, tiles))
    return win_first, ranges


class RecordLabels:
    """--labels-csv for records: a record's sample name first, then the sample of its file (`<file sample>__<id>`; the
    longest file sample that fits), so that a collection file labelled once labels all of its records.  windows: the
    samples are windows (`<record sample>__<start>-<end>`); between the two, the window's record sample is looked up."""

    def __init__(self, table, file_samples, windows=False):
        self.table = dict(table or {})
        self.file_samples = sorted(file_samples, key=len, reverse=True)
        self.windows = windows

    def get(self, sample, default=None):
        if sample in self.table:
            return self.table[sample]
        if self.windows:
            record = _WINDOW_NAME.match(sample)
            if record and record.group(1) in self.table:
                return self.table[record.group(1)]
        for fs in self.file_samples:
            if sample.startswith(fs + "__") and fs in self.table:
                return self.table[fs]
        return default


def _record_table(eng, batch, pool):
    """A batch of files in HBM and its record table: ((text, offsets, lengths), status, rec_first, bases, samples, dups,
    wanted) -- the files' status words, prefix sums of their record counts, bases and sample name of every record, the
    indices of the duplicates, and the bases again with -1 for a duplicate (what record_plan and window_plan take)."""
    dev, offs, lens = eng.upload_files(batch, pool)
    unread = getattr(eng, "last_upload_status", None)
    rec_first, _, bases, names, status = eng.fasta_records(dev, offs, lens)
    status = status.copy()
    if unread is not None:
        status[unread != 0] |= 0x100   # (a file that could not be read or inflated is not an empty sample)
    samples, dups = [], set()
    for j, f in enumerate(batch):
        a, b = int(rec_first[j]), int(rec_first[j + 1])
        got, dup = record_names(sample_of(f), names[a:b])
        samples += got
        dups.update(a + i for i in dup)
    return (dev, offs, lens), status, rec_first, bases, samples, dups, [-1 if g in dups else int(b) for g, b in enumerate(bases)]


def _record_batches(eng, files, pool, batch_bytes, min_len):
    """Per batch of files, per record: (batch, first, status, rec_first, bases, samples, dups, rows, hist, t0, t1) -- the
    files' status words, the batch's record table (prefix sums of the files' record counts, bases and sample name of
    every record, the indices of the duplicates), rows = {record: its row in hist} and hist on the device, the time the
    batch was begun and the time after the count.  One yield per call of record_plan, `first` on a batch's first, so
    that a batch whose rows pass RECORD_HIST_BYTES is imaged in pieces; a batch without a selected record yields once
    with hist None.  Records shorter than min_len and duplicates get no row."""
    import torch
    for batch, _, t0 in batches(files, batch_bytes, size=text_bytes):
        (dev, offs, lens), status, rec_first, bases, samples, dups, wanted = _record_table(eng, batch, pool)
        calls = record_plan(wanted, min_len, RECORD_HIST_BYTES, eng.ncode) or [[]]
        for n, call in enumerate(calls):
            hist = None
            if call:
                slot = np.full(len(bases), 0xFFFFFFFF, dtype=np.uint32)
                slot[call] = np.arange(len(call), dtype=np.uint32)
                hist = eng.count_fasta_records(dev, offs, lens, rec_first, slot, len(call))
                torch.cuda.current_stream(eng.device).synchronize()   # (the time after the count is the batch's)
            yield (batch, n == 0, status, rec_first, bases, samples, dups, {g: j for j, g in enumerate(call)}, hist, t0,
                   time.perf_counter())


def _record_reports(batch, status, rec_first, bases, samples, dups, min_len, stats=None, step=None):
    """What a batch's first yield says on stderr, per file: a file without records, the duplicates (each with a stats
    row `<name>#<ordinal + 1>`), how many records were passed over as too short.  step: the records are cut into
    windows of min_len bases every `step`; the line also says how many bases lie behind the records' last windows."""
    for j, f in enumerate(batch):
        a, b = int(rec_first[j]), int(rec_first[j + 1])
        if status[j] or a == b:
            eprint("K-MER COUNTING FAIL, SKIPPING FILE:", f)
            if stats is not None:
                stats.setdefault(sample_of(f), OrderedDict())["failed_step"] = "image"
            continue
        short = sum(1 for g in range(a, b) if int(bases[g]) < min_len)
        if step is not None:
            behind = sum(int(bases[g]) - (int(c) - 1) * step - min_len
                         for g, c in zip(range(a, b), window_counts(bases[a:b], min_len, step)) if c)
            eprint(f"{f}: {short} of {b - a} records shorter than {min_len} bases passed over, "
                   f"{behind} bases behind the last windows of the others")
        elif short:
            eprint(f"{f}: {short} of {b - a} records shorter than {min_len} bases passed over")
        for g in range(a, b):
            if g in dups and int(bases[g]) >= min_len:
                eprint("DUPLICATE RECORD ID, SKIPPING:", f"{samples[g]} (record {g - a + 1} of {f})")
                if stats is not None:
                    stats.setdefault(f"{samples[g]}#{g - a + 1}", OrderedDict())["failed_step"] = "image"


def _window_batches(eng, files, pool, batch_bytes, n, s):
    """Per batch of files, per row range: (batch, first, status, rec_first, bases, samples, dups, rows, hist, t0, t1) as
    _record_batches, with rows = [(record, window, its row in hist)] in row order.  One yield per range of window_plan,
    `first` on a batch's first; a batch without a window yields once with hist None.  Records shorter than n and
    duplicates get no windows."""
    import torch
    for batch, _, t0 in batches(files, batch_bytes, size=text_bytes):
        (dev, offs, lens), status, rec_first, bases, samples, dups, wanted = _record_table(eng, batch, pool)
        win_first, ranges = window_plan(wanted, n, s, WINDOW_HIST_BYTES, eng.ncode)
        chosen = np.nonzero(win_first != NO_WINDOW)[0]
        d_bases = torch.from_numpy(np.ascontiguousarray(bases).view(np.int64) if len(bases) else np.zeros(1, dtype=np.int64)).to(eng.device)
        d_first = torch.from_numpy(win_first.view(np.int64) if len(bases) else np.zeros(1, dtype=np.int64)).to(eng.device)
        for i, (lo, nrows, tile_rows) in enumerate(ranges or [None]):
            hist, rows = None, []
            if ranges:
                hist = eng.count_fasta_windows(dev, offs, lens, rec_first, d_bases, d_first, n, s, lo, nrows, tile_rows)
                torch.cuda.current_stream(eng.device).synchronize()   # (the time after the count is the batch's)
                rr = np.arange(lo, lo + nrows, dtype=np.uint64)
                gs = chosen[np.searchsorted(win_first[chosen], rr, side="right") - 1]
                rows = [(int(g), int(r - win_first[g]), j) for j, (g, r) in enumerate(zip(gs, rr))]
            yield batch, i == 0, status, rec_first, bases, samples, dups, rows, hist, t0, time.perf_counter()


def _counted(eng, files, pool, batch_bytes, genome=None, genome_rows=None):
    """Per batch of files: (batch, histograms on the device, status, bases, the time the batch was begun, after the count).
    genome (pipeline.GenomeSpectrum, `--genome-spectrum`): the same upload also goes through the assemblies' k-mer spectrum,
    behind the image count; genome_rows (a dict) receives {file: what genome.after gives for it} for the files the count
    accepts."""
    for batch, _, t0 in batches(files, batch_bytes, size=text_bytes):
        dev, offs, lens = eng.upload_files(batch, pool)
        unread = getattr(eng, "last_upload_status", None)
        hist, status, bases = eng.count_fasta(dev, offs, lens)
        st = status.cpu().numpy().copy()
        if unread is not None:
            st[unread != 0] |= 0x100   # (a file that could not be read or inflated is not an empty sample)
        t1 = time.perf_counter()
        if genome is not None:
            for j, got in enumerate(genome.after(eng, dev, offs, lens)):
                if st[j]:
                    continue   # (reported by the image count)
                if got[1]:
                    eprint("SPECTRUM FAIL:", batch[j], "- status", got[1])
                    continue
                genome_rows[batch[j]] = got
        yield batch, hist, st, bases.cpu().numpy(), t0, t1


def fasta_to_images(files, outdir, k=7, mapping_code="cgr", labels=None, device=0, rank=0, world=1, batch_bytes=None,
                    io_threads=8, engine=None, verbose=False, weights=None, fragments=False, fragment_length=150,
                    min_bp=50000, max_bp=None, seeds=None, per_record=False, min_record_length=1000, windows=False,
                    window_length=10000, window_step=None, gpu_png=False, genome=None):
    """This rank's share of FASTA `files`, each imaged whole.  Returns {sample: OrderedDict(stats)} with the reference's
    keys `<k>mer_counting_time` and `k<k>_img_time`, or `failed_step` for a sample that does not begin with '>', holds
    no base, or could not be read.

    fragments: every sample is imaged as a subsample ladder between min_bp and max_bp instead (fasta_ladder; seeds:
    {sample: int}, default 0), drawn from fragments of fragment_length bases; the stats also carry `splitting_time` and
    `splitting_bp_per_file`, and a sample whose ladder is empty gets `failed_step` = "split".

    per_record: every record of min_record_length bases or more is a sample of its own (record_names; the rule:
    INTEGRATION.md, "--from-fasta --per-record"), imaged as `image_name(<record sample>, its bases, k, mapping)`; the
    stats are keyed by record sample, `<k>mer_counting_time` is the batch's upload plus count time shared over its
    imaged records, and a record with a row but no non-zero bin gets `failed_step` = "image".

    windows: every window of window_length bases of a record, one every window_step (default: window_length), is a
    sample of its own (window_names; the rule: INTEGRATION.md, "--from-fasta --windows"), imaged as
    `image_name(<window sample>, window_length, k, mapping)`; stats and failures as for per_record, per window.

    gpu_png: the images' IDAT chunks are made on the GPU (PngSink's encoder), in every one of these modes.

    genome (pipeline.GenomeSpectrum, `--genome-spectrum`; whole files only): every sample's `<dir>/<sample>.spectrum.json`,
    counted from the upload the image is counted from, and spectrum.assembly_columns' columns in the stats."""
    files = [Path(f) for f in files]
    if genome is not None and (fragments or per_record or windows):
        raise ValueError("the genome spectrum is the whole file's: not with fragments, per_record or windows")
    if weights is None:
        weights = agreed_weights(files) if world > 1 else file_weights(files)   # (a collective when sharded)
    mine = [files[i] for i in shard_by_size(weights, rank, world)]
    stats = OrderedDict()
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        sink = PngSink(outdir, pool, k, mapping_code, labels or {}, {}, 0, eng if gpu_png else None)
        if fragments:
            for batch, _, t0 in batches(mine, batch_bytes or DEFAULT_BATCH_BYTES, size=text_bytes):
                _fragment_images(eng, pool, batch, t0, sink, stats, seeds or {}, fragment_length, min_bp, max_bp, verbose)
        if per_record:
            _record_images(eng, pool, mine, batch_bytes or DEFAULT_BATCH_BYTES, min_record_length, sink, stats, verbose)
        if windows:
            _window_images(eng, pool, mine, batch_bytes or DEFAULT_BATCH_BYTES, window_length, window_step or window_length, sink, stats,
                           verbose)
        genome_rows, reports = {}, []
        whole = () if fragments or per_record or windows else _counted(eng, mine, pool, batch_bytes or DEFAULT_BATCH_BYTES, genome,
                                                                        genome_rows)
        for batch, hist, st, bases, t0, t1 in whole:
            nz = (hist != 0).any(dim=1).cpu().numpy()
            imgs = sink.rows(eng.images(hist))
            for j, f in enumerate(batch):
                sample = sample_of(f)
                s = stats.setdefault(sample, OrderedDict())
                if f in genome_rows:
                    genome.emit(sample, genome_rows.pop(f), s, pool, reports)
                if st[j] or not nz[j]:
                    eprint("K-MER COUNTING FAIL, SKIPPING FILE:", f)
                    s["failed_step"] = "image"
                    continue
                s[str(k) + "mer_counting_time"] = (t1 - t0) / len(batch)
                sink.submit(sample, sample, image_name(sample, int(bases[j]), k, mapping_code), imgs[j])
            if verbose:
                eprint(f"batch of {len(batch)} FASTA files: upload+count {t1 - t0:.3f}s")
        for fut in reports:
            fut.result()
        sink.finish(stats)
    return stats


def _record_images(eng, pool, files, batch_bytes, min_len, sink, stats, verbose):
    """fasta_to_images(per_record=True): the record table and the selected records' rows of every batch, the images."""
    k = sink.k
    for batch, first, st, rec_first, bases, samples, dups, rows, hist, t0, t1 in _record_batches(eng, files, pool, batch_bytes, min_len):
        if first:
            _record_reports(batch, st, rec_first, bases, samples, dups, min_len, stats)
        if hist is None:
            continue
        nz = (hist != 0).any(dim=1).cpu().numpy()
        imgs = sink.rows(eng.images(hist))
        imaged = max(1, int(nz.sum()))
        for g, row in rows.items():
            s = stats.setdefault(samples[g], OrderedDict())
            if not nz[row]:
                eprint("K-MER COUNTING FAIL, SKIPPING RECORD:", samples[g])
                s["failed_step"] = "image"
                continue
            s[str(k) + "mer_counting_time"] = (t1 - t0) / imaged
            sink.submit(samples[g], samples[g], image_name(samples[g], int(bases[g]), k, sink.mapping_code), imgs[row])
        if verbose:
            eprint(f"batch of {len(batch)} FASTA files, {len(rows)} records: upload+count {t1 - t0:.3f}s")


def _window_images(eng, pool, files, batch_bytes, n, s, sink, stats, verbose):
    """fasta_to_images(windows=True): the record table and the window rows of every batch, range by range, the images."""
    k = sink.k
    for batch, first, st, rec_first, bases, samples, dups, rows, hist, t0, t1 in _window_batches(eng, files, pool, batch_bytes, n, s):
        if first:
            _record_reports(batch, st, rec_first, bases, samples, dups, n, stats, step=s)
        if hist is None:
            continue
        nz = (hist != 0).any(dim=1).cpu().numpy()
        imgs = sink.rows(eng.images(hist))
        imaged = max(1, int(nz.sum()))
        for g, w, row in rows:
            name = window_name(samples[g], n, s, w)
            stt = stats.setdefault(name, OrderedDict())
            if not nz[row]:
                eprint("K-MER COUNTING FAIL, SKIPPING WINDOW:", name)
                stt["failed_step"] = "image"
                continue
            stt[str(k) + "mer_counting_time"] = (t1 - t0) / imaged
            sink.submit(name, name, image_name(name, n, k, sink.mapping_code), imgs[row])
        if verbose:
            eprint(f"batch of {len(batch)} FASTA files, {len(rows)} windows: upload+count {t1 - t0:.3f}s")


def _fragment_images(eng, pool, batch, t0, sink, stats, seeds, frag_len, min_bp, max_bp, verbose):
    """One batch of fasta_to_images(fragments=True): upload, the ladders (one fasta_ladder call per seed), the images."""
    import torch
    k = sink.k
    dev, offs, lens = eng.upload_files(batch, pool)
    unread = getattr(eng, "last_upload_status", None)
    names = [sample_of(f) for f in batch]
    recs = [None] * len(batch)
    for seed, idx in _seed_groups(names, seeds).items():
        for j, r in zip(idx, fasta_ladder(eng, dev, offs[idx], lens[idx], frag_len, seed, min_bp, max_bp)):
            recs[j] = r
    flat = [(j, bp, h) for j, r in enumerate(recs) for bp, h, _ in r["steps"]]
    nz = torch.stack([h for _, _, h in flat]).ne(0).any(dim=1).cpu().numpy() if flat else []
    t1 = time.perf_counter()
    imgs = sink.rows(eng.images(torch.stack([h for _, _, h in flat]))) if flat else []
    for j, f in enumerate(batch):
        s = stats.setdefault(names[j], OrderedDict())
        # (a file that could not be read or inflated is not an empty sample)
        if recs[j]["status"] or recs[j]["nsites"] == 0 or (unread is not None and unread[j]):
            eprint("K-MER COUNTING FAIL, SKIPPING FILE:", f)
            s["failed_step"] = "image"
            recs[j]["steps"] = []
        elif not recs[j]["steps"]:
            eprint("SPLIT FAIL:", f, "-", recs[j]["error"] or "Input file has less than minimum data.")
            s["failed_step"] = "split"
        else:
            s["splitting_time"] = (t1 - t0) / len(batch)
            s["splitting_bp_per_file"] = ",".join(str(bp) for bp, _, _ in recs[j]["steps"])
            s[str(k) + "mer_counting_time"] = (t1 - t0) / len(batch)
    for n, (j, bp, _) in enumerate(flat):
        if not recs[j]["steps"]:
            continue
        if not nz[n]:
            eprint("IMAGE FAIL:", split_name(names[j], bp))
            stats[names[j]]["failed_step"] = "image"
            continue
        sink.submit(names[j], names[j], image_name(names[j], bp, k, sink.mapping_code), imgs[n])
    if verbose:
        eprint(f"batch of {len(batch)} FASTA files: upload+ladder {t1 - t0:.3f}s")


def fasta_to_query(samples, engine=None, k=7, mapping_code="cgr", device=0, batch_bytes=None, io_threads=8, per_record=False,
                   min_record_length=1000, origin=None, windows=False, window_length=10000, window_step=None, genome=None):
    """{sample: (bp, histogram uint32[4^k] on the device, 0)} for samples = [(sample, its FASTA file)] (this rank's
    share): what pipeline.clean_to_query returns for cleaned reads.  A sample that fails is reported and left out.

    genome (pipeline.GenomeSpectrum, `--genome-spectrum`; whole files only): every sample's `<dir>/<sample>.spectrum.json`,
    counted from the upload the histogram is counted from.

    per_record: the same tuples keyed by record sample, one per record of min_record_length bases or more
    (fasta_to_images' rule); origin (a dict) receives {record sample: the sample of its file}.

    windows: the same keyed by window sample, one per window of window_length bases every window_step, bp =
    window_length, in the order of the files, their records and the windows."""
    by_file = {Path(f): s for s, f in samples}
    found = OrderedDict()
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        if windows:
            n, s = window_length, window_step or window_length
            for batch, first, st, rec_first, bases, names, dups, rows, hist, _, _ in _window_batches(
                    eng, list(by_file), pool, batch_bytes or DEFAULT_BATCH_BYTES, n, s):
                if first:
                    _record_reports(batch, st, rec_first, bases, names, dups, n, step=s)
                if hist is None:
                    continue
                nz = (hist != 0).any(dim=1).cpu().numpy()
                file_of = np.searchsorted(rec_first, np.array([g for g, _, _ in rows], dtype=np.uint64), side="right") - 1
                for (g, w, row), j in zip(rows, file_of):
                    name = window_name(names[g], n, s, w)
                    if not nz[row]:
                        eprint("K-MER COUNTING FAIL, SKIPPING WINDOW:", name)
                        continue
                    found[name] = (n, hist[row], 0)
                    if origin is not None:
                        origin[name] = by_file[batch[int(j)]]
            return found
        if per_record:
            for batch, first, st, rec_first, bases, names, dups, rows, hist, _, _ in _record_batches(
                    eng, list(by_file), pool, batch_bytes or DEFAULT_BATCH_BYTES, min_record_length):
                if first:
                    _record_reports(batch, st, rec_first, bases, names, dups, min_record_length)
                if hist is None:
                    continue
                nz = (hist != 0).any(dim=1).cpu().numpy()
                file_of = np.searchsorted(rec_first, np.fromiter(rows, dtype=np.uint64, count=len(rows)), side="right") - 1
                for (g, row), j in zip(rows.items(), file_of):
                    if not nz[row]:
                        eprint("K-MER COUNTING FAIL, SKIPPING RECORD:", names[g])
                        continue
                    found[names[g]] = (int(bases[g]), hist[row], 0)
                    if origin is not None:
                        origin[names[g]] = by_file[batch[int(j)]]
            return found
        genome_rows, reports = {}, []
        for batch, hist, st, bases, _, _ in _counted(eng, list(by_file), pool, batch_bytes or DEFAULT_BATCH_BYTES, genome, genome_rows):
            nz = (hist != 0).any(dim=1).cpu().numpy()
            for j, f in enumerate(batch):
                if f in genome_rows:
                    genome.emit(by_file[f], genome_rows.pop(f), None, pool, reports)
                if st[j] or not nz[j]:
                    eprint("K-MER COUNTING FAIL, SKIPPING FILE:", f)
                    continue
                found[by_file[f]] = (int(bases[j]), hist[j], 0)
        for fut in reports:
            fut.result()
    return found
