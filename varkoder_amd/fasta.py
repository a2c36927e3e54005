"""`image --from-fasta` / `query --from-fasta`: assemblies, contigs, organelle genomes -- FASTA files, one sample per
file, counted whole on the GPU (ImageEngine.count_fasta; the rule: INTEGRATION.md, "--from-fasta") and imaged like any
histogram.  Stands where the reference would hand dsk a FASTA `-file` (commands/image.py:771-796).  Drawing read-like
fragments from an assembly is not done here: a sample is one image of all its bases."""
import time
from collections import OrderedDict
from pathlib import Path

from .image import eprint
from .pipeline import DEFAULT_BATCH_BYTES, PngSink, batches, engine_scope, text_bytes
from .shard import agreed_weights, file_weights, shard_by_size
from .subsample import split_name

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


def _counted(eng, files, pool, batch_bytes):
    """Per batch of files: (batch, histograms on the device, status, bases, the time the batch was begun, after the count)."""
    for batch, _, t0 in batches(files, batch_bytes, size=text_bytes):
        dev, offs, lens = eng.upload_files(batch, pool)
        unread = getattr(eng, "last_upload_status", None)
        hist, status, bases = eng.count_fasta(dev, offs, lens)
        st = status.cpu().numpy().copy()
        if unread is not None:
            st[unread != 0] |= 0x100   # (a file that could not be read or inflated is not an empty sample)
        yield batch, hist, st, bases.cpu().numpy(), t0, time.perf_counter()


def fasta_to_images(files, outdir, k=7, mapping_code="cgr", labels=None, device=0, rank=0, world=1, batch_bytes=None,
                    io_threads=8, engine=None, verbose=False, weights=None):
    """This rank's share of FASTA `files`, each imaged whole.  Returns {sample: OrderedDict(stats)} with the reference's
    keys `<k>mer_counting_time` and `k<k>_img_time`, or `failed_step` for a sample that does not begin with '>', holds
    no base, or could not be read."""
    files = [Path(f) for f in files]
    if weights is None:
        weights = agreed_weights(files) if world > 1 else file_weights(files)   # (a collective when sharded)
    mine = [files[i] for i in shard_by_size(weights, rank, world)]
    stats = OrderedDict()
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        sink = PngSink(outdir, pool, k, mapping_code, labels or {}, {}, 0)
        for batch, hist, st, bases, t0, t1 in _counted(eng, mine, pool, batch_bytes or DEFAULT_BATCH_BYTES):
            nz = (hist != 0).any(dim=1).cpu().numpy()
            imgs = eng.images(hist).cpu().numpy()
            for j, f in enumerate(batch):
                sample = sample_of(f)
                s = stats.setdefault(sample, OrderedDict())
                if st[j] or not nz[j]:
                    eprint("K-MER COUNTING FAIL, SKIPPING FILE:", f)
                    s["failed_step"] = "image"
                    continue
                s[str(k) + "mer_counting_time"] = (t1 - t0) / len(batch)
                sink.submit(sample, sample, image_name(sample, int(bases[j]), k, mapping_code), imgs[j])
            if verbose:
                eprint(f"batch of {len(batch)} FASTA files: upload+count {t1 - t0:.3f}s")
        sink.finish(stats)
    return stats


def fasta_to_query(samples, engine=None, k=7, mapping_code="cgr", device=0, batch_bytes=None, io_threads=8):
    """{sample: (bp, histogram uint32[4^k] on the device, 0)} for samples = [(sample, its FASTA file)] (this rank's
    share): what pipeline.clean_to_query returns for cleaned reads.  A sample that fails is reported and left out."""
    by_file = {Path(f): s for s, f in samples}
    found = OrderedDict()
    with engine_scope(engine, k, mapping_code, device, io_threads) as (eng, pool):
        for batch, hist, st, bases, _, _ in _counted(eng, list(by_file), pool, batch_bytes or DEFAULT_BATCH_BYTES):
            nz = (hist != 0).any(dim=1).cpu().numpy()
            for j, f in enumerate(batch):
                if st[j] or not nz[j]:
                    eprint("K-MER COUNTING FAIL, SKIPPING FILE:", f)
                    continue
                found[by_file[f]] = (int(bases[j]), hist[j], 0)
    return found
