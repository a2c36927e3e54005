"""`image / query --from-bam`: the host half.  A .bam is BGZF: its bytes are uploaded and inflated in HBM like any gzip
file (ImageEngine.upload_files) and converted to FASTQ text there (ImageEngine.bam_to_fastq: csrc/vk_bam.h).  What the
device needs from the host is where each file's first record starts and how many references its header names; that is
all this module reads of a file (the rule: INTEGRATION.md, "--from-bam: the rule"; SAM spec section 4.2)."""
import mmap
import os
import struct
import zlib
from pathlib import Path

from . import _capi

BAM_SUFFIX = ".bam"
EXCLUDE_DEFAULT = 0x900   # secondary, supplementary: `samtools fastq`'s default
FASTQ_SLACK = 4096        # bytes on top of 4/3 of the inflated size in a batch's estimate


class BamError(Exception):
    """A file that is not BAM, or whose header does not parse."""


def sample_of(path):
    """The sample a BAM file holds: its name up to `.bam` (in either case); None: not one."""
    name = Path(path).name
    return name[:-len(BAM_SUFFIX)] if name.lower().endswith(BAM_SUFFIX) and len(name) > len(BAM_SUFFIX) else None


def bam_files(src):
    """The BAM files of folder `src`, sorted by name; two files of one sample are an error."""
    files = sorted(f for f in Path(src).iterdir() if f.is_file() and sample_of(f) is not None)
    seen = {}
    for f in files:
        s = sample_of(f)
        if s in seen:
            raise Exception(f"Two BAM files for sample {s}: {seen[s].name} and {f.name}")
        seen[s] = f
    return files


def _members(fh, size):
    """(offset, compressed size, text size) of the BGZF members of an open file, one after another, by the 18-byte header
    rule of engine.bgzf_members; BamError where the file stops being BGZF."""
    pos = 0
    while pos < size:
        fh.seek(pos)
        h = fh.read(18)
        if (len(h) < 18 or h[0] != 0x1F or h[1] != 0x8B or h[2] != 8 or not (h[3] & 4) or h[10] != 6 or h[11] != 0
                or h[12:16] != b"BC\x02\x00"):
            raise BamError("not BGZF")
        bsize = (h[16] | (h[17] << 8)) + 1
        if bsize < 26 or pos + bsize > size:
            raise BamError("a BGZF member runs past the file's end")
        fh.seek(pos + bsize - 4)
        text = int.from_bytes(fh.read(4), "little")
        if text > 65536:
            raise BamError("a BGZF member of more than 64 KiB of text")
        yield pos, bsize, text
        pos += bsize


class _Head:
    """The first bytes of a BAM file's text, inflated member by member as far as they are asked for.  need(n) makes n
    bytes available or raises: before anything is inflated for it, the members' own size words must add up to n, so a
    length field that points past the file costs a walk over block headers and no memory."""

    def __init__(self, fh, size):
        self.fh, self.buf = fh, bytearray()
        self.members = _members(fh, size)
        self.ahead = []        # members hopped over and not yet inflated
        self.known = 0         # text bytes of every member hopped over so far

    def need(self, n):
        while self.known < n:
            m = next(self.members, None)
            if m is None:
                raise BamError("the header points past the file's end")
            self.ahead.append(m)
            self.known += m[2]
        while len(self.buf) < n:
            pos, bsize, text = self.ahead.pop(0)
            self.fh.seek(pos + 18)
            raw = self.fh.read(bsize - 26)
            try:
                got = zlib.decompress(raw, wbits=-15, bufsize=max(text, 1))
            except zlib.error as e:
                raise BamError(f"a BGZF member does not inflate: {e}") from None
            if len(got) != text:
                raise BamError("a BGZF member's size word does not match its text")
            self.buf += got

    def i32(self, at):
        self.need(at + 4)
        return struct.unpack_from("<i", self.buf, at)[0]


def _header(path):
    """(first_record, n_ref, the header's text) of a BAM file: bam_header and read_groups parse it."""
    size = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = _Head(fh, size)
        head.need(4)
        if bytes(head.buf[:4]) != b"BAM\x01":
            raise BamError("no BAM magic")
        l_text = head.i32(4)
        if l_text < 0:
            raise BamError("negative l_text")
        head.need(8 + l_text)
        text = bytes(head.buf[8:8 + l_text])
        at = 8 + l_text
        n_ref = head.i32(at)
        at += 4
        if n_ref < 0:
            raise BamError("negative n_ref")
        head.need(at + 8 * n_ref)   # (a reference takes at least l_name and l_ref)
        for _ in range(n_ref):
            l_name = head.i32(at)
            if l_name < 0:
                raise BamError("negative l_name")
            head.need(at + 4 + l_name + 4)
            at += 8 + l_name
    return at, n_ref, text


def bam_header(path):
    """(first_record, n_ref, sort_order) of a BAM file: the offset of its first record in the inflated bytes, the
    references its header names and what its `@HD` line says behind `SO:` ("unknown" without one).  Only the BGZF members
    the header lies in are inflated (zlib).  BamError for a file that is not BAM or whose header does not parse."""
    at, n_ref, text = _header(path)
    return at, n_ref, _sort_order(text)


def _sort_order(text):
    order = "unknown"
    first = text.split(b"\n", 1)[0]
    if first.startswith(b"@HD"):
        for field in first.split(b"\t")[1:]:
            if field.startswith(b"SO:"):
                order = field[3:].rstrip(b"\r\0").decode("latin-1")
    return order


MAX_GROUPS = _capi.VK_BAM_MAX_GROUPS
MAX_ID_BYTES = 255
GROUP_ID_BYTES = 100   # of a group's id in its sample name (fasta.RECORD_ID_BYTES)


def groups_of_text(text):
    """The read groups of a header's text: the `ID:` fields (bytes) of its `@RG` lines, in header order (SAM spec 1.3).
    BamError for an `@RG` line without `ID:` (or with an empty one), an ID of more than 255 bytes, an ID twice, more than
    VK_BAM_MAX_GROUPS groups."""
    ids, seen = [], set()
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r\0")
        if line != b"@RG" and not line.startswith(b"@RG\t"):
            continue
        rid = next((f[3:] for f in line.split(b"\t")[1:] if f.startswith(b"ID:")), b"")
        if not rid:
            raise BamError("an @RG line without ID:")
        if len(rid) > MAX_ID_BYTES:
            raise BamError("a read group ID of more than %d bytes" % MAX_ID_BYTES)
        if rid in seen:
            raise BamError("read group ID %s twice" % rid.decode("latin-1"))
        seen.add(rid)
        ids.append(rid)
        if len(ids) > MAX_GROUPS:
            raise BamError("more than %d read groups" % MAX_GROUPS)
    return ids


def read_groups(path):
    """The read groups of a BAM file (groups_of_text of its header), read once per file as it stands on disk (cached
    beside file_info, by its key); BamError as bam_header raises it, or for a header whose @RG lines break the rule
    ("--from-bam --bam-read-groups: the rule")."""
    st = os.stat(path)
    key = (str(path), st.st_size, st.st_mtime_ns)
    if key not in _GROUPS:
        try:
            _GROUPS[key] = groups_of_text(_header(path)[2])
        except (BamError, ValueError) as e:
            _GROUPS[key] = BamError(str(e) or type(e).__name__)
    if isinstance(_GROUPS[key], BamError):
        raise _GROUPS[key]
    return list(_GROUPS[key])


def group_names(file_sample, ids):
    """The sample names of a file's groups: `<file sample>__<id>`, the id cleaned and cut as fasta.record_names cleans a
    record's (every byte outside [A-Za-z0-9._-] replaced by '_', at most GROUP_ID_BYTES).  BamError when two groups of
    the file come to one name."""
    out, seen = [], {}
    for rid in ids:
        clean = "".join(chr(b) if (48 <= b <= 57 or 65 <= b <= 90 or 97 <= b <= 122 or b in b"._-") else "_"
                        for b in bytes(rid)[:GROUP_ID_BYTES])
        name = f"{file_sample}__{clean}"
        if name in seen:
            raise BamError("read groups %s and %s both give the sample %s" % (seen[name].decode("latin-1"),
                                                                               bytes(rid).decode("latin-1"), name))
        seen[name] = bytes(rid)
        out.append(name)
    return out


_INFO = {}   # (path, size, mtime) -> (inflated size, header) or the BamError
_GROUPS = {}   # the same key -> the read groups or the BamError


def file_info(path):
    """(inflated size, (first_record, n_ref, sort_order)) of a BAM file, read once per file as it stands on disk (its
    size and modification time): the batcher, the sort-order check and the upload all ask.  BamError as inflated_size and
    bam_header raise it."""
    st = os.stat(path)
    key = (str(path), st.st_size, st.st_mtime_ns)
    if key not in _INFO:
        try:
            _INFO[key] = (inflated_size(path), bam_header(path))
        except (BamError, ValueError) as e:
            _INFO[key] = BamError(str(e) or type(e).__name__)
    if isinstance(_INFO[key], BamError):
        raise _INFO[key]
    return _INFO[key]


def inflated_size(path):
    """Bytes of a BAM file once inflated (engine.bgzf_text_size); BamError when it is not BGZF from end to end."""
    from .engine import bgzf_text_size
    if os.path.getsize(path) == 0:
        raise BamError("empty file")
    with open(path, "rb") as fh, mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
        n = bgzf_text_size(mm)
    if n is None:
        raise BamError("not BGZF")
    return n


def batch_bytes(path):
    """What a BAM file takes of a batch in HBM: its inflated bytes and the FASTQ text made of them.  A read's text is
    l_read_name + 2 * l_seq + 5 bytes out of a record of at least 36 + l_read_name + 1.5 * l_seq: at most 4/3 of it.  A
    file that cannot be sized counts its size on disk (it fails later, with a report)."""
    try:
        n = file_info(path)[0]
    except (BamError, OSError):
        return os.path.getsize(path) if os.path.exists(path) else 0
    return n + n * 4 // 3 + FASTQ_SLACK


def sample_plan(path, pairs=False, group=None):
    """A sample's streams [(file, role, select)] in the order step B reads a sample's files (pipeline._sample_files):
    single-end first, then R1, then R2.  group (`--bam-read-groups`: an index into read_groups(path), or
    VK_BAM_UNGROUPED): [(file, role, select, group)], the streams of that group's reads."""
    more = () if group is None else (group,)
    if not pairs:
        return [(path, _capi.VK_CL_ROLE_UNPAIRED, _capi.VK_BAM_ALL) + more]
    return [(path, _capi.VK_CL_ROLE_UNPAIRED, _capi.VK_BAM_SINGLE) + more, (path, _capi.VK_CL_ROLE_R1, _capi.VK_BAM_READ1) + more,
            (path, _capi.VK_CL_ROLE_R2, _capi.VK_BAM_READ2) + more]


def group_samples(files):
    """`--bam-read-groups`: ([(sample, file, group index)] for every group of every file, in file and header order,
    {file: why it has no samples}).  A file that is not BAM or whose @RG lines break the rule has none (the reason is
    reported, the run goes on); a file without @RG lines has none either.  A group sample that is also another file's
    sample or another file's group sample is the error that two BAM files of one sample are."""
    out, why = [], {}
    taken = {sample_of(f): f for f in files}
    for f in files:
        try:
            ids = read_groups(f)
            names = group_names(sample_of(f), ids)
        except (BamError, OSError) as e:
            why[f] = str(e) or type(e).__name__
            continue
        if not ids:
            why[f] = "no @RG line in the header: no read groups, no samples"
        for g, name in enumerate(names):
            if name in taken:
                raise Exception(f"Two BAM files for sample {name}: {Path(taken[name]).name} and {Path(f).name}")
            taken[name] = f
            out.append((name, f, g))
    return out, why


def check_pairs(files):
    """`--bam-pairs` relies on mates in the same order: a file whose header says SO:coordinate is refused.  Returns the
    message, or None.  (A file whose header does not parse is left to the run: it fails its own sample.)"""
    for f in files:
        try:
            order = file_info(f)[1][2]
        except (BamError, OSError):
            continue
        if order == "coordinate":
            return f"--bam-pairs: {f} is sorted by coordinate (SO:coordinate); collate it by name first"
    return None
