"""Device-resident batch interface to the HIP kernels (one process per GPU).

PyTorch is used for device memory and the stream only; every computation is a call
through the C ABI of include/vkimg.h.  There is no CPU fallback.
"""
import ctypes as C
import mmap
import os
import sys

import numpy as np

from . import _capi
from .config import KMER_MAX, KMER_MIN
from .mapping import pixel_lut, side


def _torch():
    import torch
    return torch


def _u64(a):
    """A NumPy array's data as the C ABI takes it: uint64_t*; _u32, _u8 alike."""
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def bgzf_members(buf):
    """The members of a BGZF file (what `bgzip` and BBTools-through-bgzip write: gzip members of at most
    64 KiB, each with its own size in a 'BC' extra field), found by hopping from block header to block header
    -- no inflating: (offsets, compressed sizes, text sizes) as uint64 arrays, or None when `buf` is not BGZF
    from end to end.  The last member of such a file is an empty one (ISIZE 0), so the size word that ends
    the FILE says nothing about the text; and since no member refers to another, every member can be inflated
    by a wavefront of its own."""
    n = len(buf)
    if n == 0:
        return None
    mv = memoryview(buf)
    offs, sizes, texts = [], [], []
    pos = 0
    while pos < n:
        if pos + 18 > n:
            return None
        h = bytes(mv[pos:pos + 18])
        if h[0] != 0x1F or h[1] != 0x8B or h[2] != 8 or not (h[3] & 4) or h[10] != 6 or h[11] != 0 or h[12:16] != b"BC\x02\x00":
            return None
        size = (h[16] | (h[17] << 8)) + 1
        if size < 26 or pos + size > n:
            return None
        text = int.from_bytes(bytes(mv[pos + size - 4:pos + size]), "little")
        if text > 65536:     # a BGZF block holds at most 64 KiB of text: anything else is not BGZF (or hostile) and
            return None      # goes the ordinary way, whose text slot is clamped against the file's size on disk
        offs.append(pos)
        sizes.append(size)
        texts.append(text)
        pos += size
    return (np.array(offs, dtype=np.uint64), np.array(sizes, dtype=np.uint64), np.array(texts, dtype=np.uint64))


def bgzf_text_size(buf):
    """Text bytes of a BGZF file (the sum of its members' ISIZE words), None when `buf` is not BGZF."""
    m = bgzf_members(buf)
    return None if m is None else int(m[2].sum())


# A gzip file's text slot in HBM is reserved before anything is inflated.  The size word that ends the file
# (ISIZE) is the size of its LAST member modulo 2^32 -- right for what split_fastq writes, arbitrary bytes
# in a truncated file: never reserve more than this many times the file's size on disk (+ slack); a file
# that really expands further overflows its slot and is inflated again into one of the size the first pass
# reported (vk_inflate_device, VK_GZ_OVERFLOW).
GZ_MAX_FIRST_RATIO = 64
# How plain-text files reach the GPU: mapped and copied by DMA straight out of the page cache (stage_files /
# vk_upload_mapped: next to no host work) or read() into the pinned staging buffer by the I/O threads (a core per
# ~3 GB/s).  With 16 threads the second is 3-7 % faster on one GPU (both run at the link's rate; measured, DESIGN.md
# 5); a rank that has fewer -- several ranks sharing a host's cores -- cannot feed its link that way.
# VARKODER_AMD_MMAP=1 / 0 forces one or the other; unset: mapped when the rank has fewer than MAPPED_BELOW_THREADS.
USE_MAPPED_UPLOAD = {"1": True, "0": False}.get(os.environ.get("VARKODER_AMD_MMAP", ""))
MAPPED_BELOW_THREADS = 16
# ImageEngine.png: output and workspace of one vk_png_device call at most (a --windows batch of 100,000 images of
# 16 KiB would otherwise ask for 3.4 GB at once)
PNG_CALL_BYTES = 512 << 20


def slots16(sizes):
    """Slots for texts of `sizes` bytes one after another, each at a multiple of 16 bytes (as upload() lays samples out):
    (offsets uint64, the bytes of all slots together)."""
    rounded = (np.asarray(sizes, dtype=np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    offs = np.zeros(len(rounded), dtype=np.uint64)
    if len(rounded) > 1:
        offs[1:] = np.cumsum(rounded[:-1])
    return offs, int(rounded.sum())


def _bam_group_args(nfiles, groups):
    """groups: per file the list of its group IDs (bytes) -> (group_first uint32 [nfiles + 1], id_first uint32
    [groups + 1], the ID bytes uint8 (never empty: ctypes wants an address))."""
    groups = [list(g) for g in groups]
    if len(groups) != nfiles:
        raise ValueError("groups: one list of IDs per file")
    gfirst = np.zeros(nfiles + 1, dtype=np.uint32)
    gfirst[1:] = np.cumsum([len(g) for g in groups])
    ids = [bytes(i) for g in groups for i in g]
    ifirst = np.zeros(len(ids) + 1, dtype=np.uint32)
    ifirst[1:] = np.cumsum([len(i) for i in ids])
    raw = np.frombuffer(b"".join(ids) + b"\0", dtype=np.uint8).copy()
    return gfirst, ifirst, raw


def bam_groups_workspace_size(lengths, groups, stream_file, seg_bytes=0, panel_segs=0, L=None):
    """Bytes of workspace vk_bam_groups_frame_device / vk_bam_groups_fastq_device take beyond the ungrouped calls
    (vk_bam_groups_workspace_size: host only, no context) for files of `lengths` inflated bytes whose groups are
    groups[i] (a list of IDs), streams of the files `stream_file`, segments of seg_bytes and panels of panel_segs segments
    (0: the defaults)."""
    L = L or _capi.lib()
    lens = np.ascontiguousarray(lengths, dtype=np.uint64)
    sf = np.ascontiguousarray(stream_file, dtype=np.uint32)
    gfirst, ifirst, _ = _bam_group_args(len(lens), groups)
    out = C.c_uint64()
    st = L.vk_bam_groups_workspace_size(_u64(lens), len(lens), _u32(gfirst), _u32(ifirst), _u32(sf), len(sf), int(seg_bytes),
                                        int(panel_segs), C.byref(out))
    if st:
        raise _capi.VkError(st, "vk_bam_groups_workspace_size")
    return out.value


def plain_route(threads, engine=None):
    """"mapped" or "staged": how stage_files brings plain-text files in for a rank with this many I/O threads.
    VARKODER_AMD_MMAP decides when set; else what the engine's pipeline has switched to (ImageEngine.route_override:
    pipeline.fastqs_to_images goes over to the mapped route when its staging threads -- read() into pinned memory -- keep
    the copy engine waiting); else mapped below MAPPED_BELOW_THREADS threads."""
    if USE_MAPPED_UPLOAD is not None:
        return "mapped" if USE_MAPPED_UPLOAD else "staged"
    if engine is not None and getattr(engine, "route_override", None) in ("mapped", "staged"):
        return engine.route_override
    return "mapped" if threads < MAPPED_BELOW_THREADS else "staged"


class ScreenSet:
    """The k-mer set of a screen's reference as ImageEngine.screen_set leaves it in HBM: the table (an int64 device
    tensor of `slots` words, a free slot all ones), its k, the distinct keys it holds and the windows they came from.
    The table is freed with the object."""

    def __init__(self, table, slots, k, distinct, windows):
        self.table, self.slots, self.k, self.distinct, self.windows = table, slots, k, distinct, windows

    def keys(self):
        """The keys as a sorted uint64 array on the host (tests)."""
        t = self.table.cpu().numpy().view(np.uint64)
        return np.sort(t[t != np.uint64(0xFFFFFFFFFFFFFFFF)])


class ImageEngine:
    """FASTQ (in HBM) -> forward k-mer histograms -> uint8 images, for one k and mapping.

    Mirrors steps D+E of run_clean2img (varKoder/commands/image.py:1054-1127) for a
    batch of samples that are already resident on the GPU.
    """

    def __init__(self, k=7, mapping="cgr", device=0, lut=None, npix=None):
        if k not in range(KMER_MIN, KMER_MAX + 1):
            raise ValueError("kmer size must be between 5 and 9")
        torch = _torch()
        if not torch.cuda.is_available():
            raise _capi.VkError(_capi.VK_EHIP, "no GPU visible: the HIP path cannot run (no CPU fallback)")
        self.k = k
        self.mapping = mapping
        self.route_override = None   # see plain_route
        self.device = torch.device("cuda", device)
        self.L = _capi.lib()
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.current_stream(self.device)
        ctx = C.c_void_p()
        _capi.check(None, self.L.vk_ctx_create(device, C.c_void_p(self.stream.cuda_stream), 0, C.byref(ctx)),
                    "vk_ctx_create")
        self.ctx = ctx
        if lut is None:
            self.side = side(k, mapping)
            self.npix = self.side * self.side
            if mapping == "cgr":
                st = self.L.vk_set_mapping(self.ctx, k, None, self.npix)
            else:
                lut = np.ascontiguousarray(pixel_lut(k, mapping), dtype=np.uint32)
                st = self.L.vk_set_mapping(self.ctx, k, _u32(lut), self.npix)
        else:
            lut = np.ascontiguousarray(lut, dtype=np.uint32)
            self.npix = int(npix)
            self.side = int(round(self.npix ** 0.5))
            st = self.L.vk_set_mapping(self.ctx, k, _u32(lut), self.npix)
        _capi.check(self.ctx, st, "vk_set_mapping")
        self.ncode = 4 ** k

    def close(self):
        ex = self.__dict__.pop("_releaser", None)
        if ex is not None:
            ex.shutdown(wait=True)   # mapped files still being unpinned
        self.__dict__.pop("screen_sets", None)   # (the tables of pipeline.Screen: freed with the engine)
        if getattr(self, "ctx", None):
            self.L.vk_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------
    @staticmethod
    def _desc(offsets, lengths):
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lengths, dtype=np.uint64)
        if offs.shape != lens.shape or offs.ndim != 1:
            raise ValueError("offsets and lengths must be 1-D and of equal length")
        return offs, lens

    def _ptr(self, t):
        return C.c_void_p(t.data_ptr())

    def upload(self, samples):
        """Pack host FASTQ byte strings into one device buffer at 16-byte aligned offsets;
        returns (tensor, offsets, lengths).  The bytes go through a pinned staging buffer that
        is kept (and grown) across calls, so the H2D copy is a single DMA at link speed."""
        torch = _torch()
        lens = np.array([len(s) for s in samples], dtype=np.uint64)
        offs = np.zeros(len(samples), dtype=np.uint64)
        pos = 0
        for i, n in enumerate(lens):
            offs[i] = pos
            pos += (int(n) + 15) // 16 * 16
        total = pos + 16
        pinned = getattr(self, "_pinned", None)
        if pinned is None or pinned.numel() < total:
            pinned = torch.empty(max(total, 1 << 20), dtype=torch.uint8, pin_memory=True)
            self._pinned = pinned
        host = pinned.numpy()
        for s, o, n in zip(samples, offs, lens):
            o, n = int(o), int(n)
            host[o:o + n] = np.frombuffer(s, dtype=np.uint8) if not isinstance(s, np.ndarray) else s
            host[o + n:(o + n + 15) // 16 * 16] = 0
        host[pos:total] = 0
        dev = torch.empty(total, dtype=torch.uint8, device=self.device)
        dev.copy_(pinned[:total], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()   # the staging buffer is reused
        return dev, offs, lens

    def h2d_link_rate(self):
        """Bytes per second of a pinned -> device copy on this engine's device (128 MiB, best of three; measured once)."""
        if getattr(self, "_h2d_rate", None) is None:
            import time
            torch = _torch()
            n = 128 << 20
            src = torch.empty(n, dtype=torch.uint8).pin_memory()
            dst = torch.empty(n, dtype=torch.uint8, device=self.device)
            best = 0.0
            for _ in range(3):
                torch.cuda.synchronize(self.device)
                t0 = time.perf_counter()
                dst.copy_(src, non_blocking=True)
                torch.cuda.synchronize(self.device)
                best = max(best, n / (time.perf_counter() - t0))
            self._h2d_rate = best
            del src, dst
        return self._h2d_rate

    def stage_files(self, paths, pool=None, slot=0):
        """Host half of upload_files: read the files, AS THEY ARE ON DISK, into pinned staging buffer
        `slot` (kept and grown across calls) with parallel readinto, no intermediate copy.  Plain FASTQ
        files land at their final 16-byte aligned text offsets; gzip files (what step C of the
        reference writes, commands/image.py:696-708) stay compressed -- they cross PCIe that way and
        are inflated on the GPU by upload_staged -- and only get their text slot reserved (its size is
        the ISIZE word that ends a gzip file).  May run on a thread of its own (a pipeline stages the
        next batch while this one is copied and processed): the only GPU-runtime call is the pinned
        allocation, made with this engine's device current.  A file that cannot be read is staged with
        length 0 -- the caller sees an empty histogram for it and skips it as the reference skips a
        file dsk fails on (commands/image.py:1070-1075) -- and never takes the batch with it."""
        import os
        torch = _torch()
        torch.cuda.set_device(self.device)  # thread-local: a fresh thread would otherwise allocate on device 0

        def probe(p):
            """(is_gzip, bytes on disk, text bytes expected)"""
            try:
                size = os.path.getsize(p)
                with open(p, "rb") as f:
                    gz = f.read(2) == b"\x1f\x8b"
                    if not gz:
                        return False, size, size
                    if size < 18:
                        return True, 0, 0
                    f.seek(size - 4)
                    return True, size, int.from_bytes(f.read(4), "little")
            except OSError as e:
                print("cannot read", str(p) + ":", repr(e), file=sys.stderr)
                return False, 0, 0
        mapper = pool.map if pool is not None else map
        info = list(mapper(probe, paths))
        n = len(paths)
        is_gz = np.array([g for g, _, _ in info], dtype=bool)
        disk = np.array([d for _, d, _ in info], dtype=np.uint64)
        unreadable = np.zeros(n, dtype=bool)   # files that exist on the command line but could not be read
        for i, p in enumerate(paths):
            if int(disk[i]) == 0:
                try:
                    unreadable[i] = os.path.getsize(p) != 0    # (a gzip file under 18 bytes is not one)
                except OSError:
                    unreadable[i] = True
        lens = np.array([0 if g else t for g, _, t in info], dtype=np.uint64)      # gzip: known after the inflate
        caps = np.array([t for _, _, t in info], dtype=np.uint64)                  # text slot sizes
        for i in np.flatnonzero(is_gz):
            caps[i] = min(int(caps[i]), GZ_MAX_FIRST_RATIO * int(disk[i]) + (1 << 16))
        # staging layout: the plain files at their final 16-byte aligned text offsets, then the compressed files
        offs = np.zeros(n, dtype=np.uint64)
        pos = 0
        for i in np.flatnonzero(~is_gz):
            offs[i] = pos
            pos += (int(caps[i]) + 15) // 16 * 16
        plain_total = pos
        src = np.zeros(n, dtype=np.uint64)
        src[~is_gz] = offs[~is_gz]
        for i in np.flatnonzero(is_gz):
            src[i] = pos
            pos += (int(disk[i]) + 15) // 16 * 16
        # Plain files are not read at all where the platform allows it: they are mapped (MAP_SHARED, populated here,
        # on the staging threads) and upload_staged has the GPU copy them straight out of the page cache
        # (vk_upload_mapped) -- the read() into the pinned buffer, at ~3 GB/s per core, was what bounded plain-text
        # input, not the 57 GB/s link.  A file that cannot be mapped goes through the buffer as before.
        mapped = {}
        threads = getattr(pool, "_max_workers", 1) if pool is not None else 1
        if plain_route(threads, self) == "mapped":
            def map_file(i):
                if int(disk[i]) == 0:
                    return None
                if is_gz[i] and (int(disk[i]) < 28 or int(disk[i]) % 4096 == 0 or int(disk[i]) % 4096 > 4032):
                    return None   # (the inflate kernels read a compressed file in place: its last page keeps room behind the end)
                try:
                    fd = os.open(paths[i], os.O_RDONLY)
                    try:
                        if os.fstat(fd).st_size != int(disk[i]):
                            return None
                        mm = mmap.mmap(fd, int(disk[i]), flags=mmap.MAP_SHARED | getattr(mmap, "MAP_POPULATE", 0),
                                       prot=mmap.PROT_READ)
                    finally:
                        os.close(fd)
                except (OSError, ValueError):
                    return None
                view = np.frombuffer(mm, dtype=np.uint8)
                # pinned for the DMA engines here, ahead of the copy and beside it (upload_staged pins what is not)
                ctx = getattr(self, "ctx", None)
                pinned_now = bool(ctx) and self.L.vk_host_register(ctx, C.c_void_p(view.ctypes.data), view.size) == _capi.VK_OK
                if is_gz[i] and not pinned_now:   # kernels cannot read what is not pinned: through the staging buffer
                    view = None
                    mm.close()
                    return None
                return [mm, view, pinned_now]
            for i, m in enumerate(mapper(map_file, range(n))):
                if m is not None:
                    mapped[i] = m
        stage_total = pos + 16
        slots = self.__dict__.setdefault("_pinned_slots", {})
        pinned = slots.get(slot)
        if pinned is None or pinned.numel() < stage_total:
            pinned = torch.empty(max(stage_total, 1 << 20), dtype=torch.uint8, pin_memory=True)
            slots[slot] = pinned
        host = pinned.numpy()
        bgzf = {}    # file index -> member table of a BGZF file

        def fill(i):
            o, nb = int(src[i]), int(disk[i])
            got = 0
            if i in mapped:
                view = mapped[i][1]
                if is_gz[i] and view[3] & 4:
                    m = bgzf_members(view)
                    if m is not None:
                        caps[i] = int(m[2].sum())
                        bgzf[i] = m
                return
            if nb:
                try:
                    with open(paths[i], "rb") as f:
                        got = f.readinto(memoryview(host[o:o + nb]))
                except OSError as e:
                    print("cannot read", str(paths[i]) + ":", repr(e), file=sys.stderr)
                    got = -1
                if got != nb:      # unreadable or changed under us: an empty sample, not a dead batch
                    disk[i] = 0
                    lens[i] = 0
                    caps[i] = 0
                    unreadable[i] = True
                elif is_gz[i] and nb >= 28 and host[o + 3] & 4:
                    # many-member files (BGZF): the text size is the sum over the members, found by walking
                    # the block headers -- not the last member's size word (0 for BGZF's empty end marker)
                    m = bgzf_members(host[o:o + nb])
                    if m is not None:
                        caps[i] = int(m[2].sum())
                        bgzf[i] = m
            host[o + nb:(o + nb + 15) // 16 * 16] = 0
        list(mapper(fill, range(n)))
        # text layout in HBM: the plain region as staged, then the slots of the gzip files
        pos = plain_total
        for i in np.flatnonzero(is_gz):
            offs[i] = pos
            pos += (int(caps[i]) + 15) // 16 * 16
        text_total = pos + 16
        return {"pinned": pinned, "plain_total": plain_total, "stage_total": stage_total, "text_total": text_total,
                "is_gz": is_gz, "src": src, "disk": disk, "offs": offs, "lens": lens, "caps": caps,
                "paths": [str(p) for p in paths], "bgzf": bgzf, "mapped": mapped, "unreadable": unreadable,
                "plain_route": "mapped" if any(not is_gz[i] for i in mapped) else "staged"}

    def _release_mapped(self, mapped, which=None):
        """Unpin and unmap files of a batch (all, or those named) -- on a helper thread: it is a few milliseconds per
        batch that nothing has to wait for (close() waits for it)."""
        keys = list(mapped) if which is None else list(which)
        items = [mapped.pop(i) for i in keys]
        ctx, L = self.ctx, self.L

        def work():
            for m in items:
                mm, view, pinned_now = m
                if pinned_now:
                    L.vk_host_unregister(ctx, C.c_void_p(view.ctypes.data))
                m[1] = view = None
                try:
                    mm.close()
                except BufferError:
                    pass
        ex = self.__dict__.get("_releaser")
        if ex is None:
            from concurrent.futures import ThreadPoolExecutor
            ex = self.__dict__["_releaser"] = ThreadPoolExecutor(1)
        ex.submit(work)

    def upload_staged(self, staged, timings=None):
        """Device half: one H2D DMA of the plain text, one of the compressed files, and the gzip files
        inflated in HBM into their text slots (vk_inflate_device).  Returns (tensor, offsets, lengths);
        the staging buffer may be refilled once this returns.  A gzip file the GPU rejects (bad header
        or data, truncated, size word or CRC-32 wrong) gets length 0 and a line on stderr."""
        mapped = staged.get("mapped") or {}
        try:
            return self._upload_staged(staged, mapped, timings)
        finally:
            if mapped:      # also when a call in there raised: the files' pages must not stay pinned
                self._release_mapped(mapped)

    def _upload_staged(self, staged, mapped, timings):
        torch = _torch()
        pinned, plain_total, stage_total = staged["pinned"], staged["plain_total"], staged["stage_total"]
        offs, lens, is_gz = staged["offs"], staged["lens"].copy(), staged["is_gz"]
        # per file: 0 = its text is in HBM (possibly empty), VK_GZ_* bits of a failed inflate, 0x100 = unreadable
        fstat = np.where(staged.get("unreadable", np.zeros(len(offs), dtype=bool)), 0x100, 0).astype(np.uint32)
        self.last_upload_status = fstat
        idx = [i for i in sorted(mapped) if not is_gz[i]]
        if idx:
            # (zeroed: a mapped file brings no padding up to its 16-byte rounded end along)
            dev = torch.zeros(staged["text_total"], dtype=torch.uint8, device=self.device)
            views = [mapped[i][1] for i in idx]
            srcp = (C.c_void_p * len(idx))(*[v.ctypes.data for v in views])
            flags = np.array([1 if mapped[i][2] else 0 for i in idx], dtype=np.uint8)
            st = np.zeros(len(idx), dtype=np.uint32)
            _capi.check(self.ctx, self.L.vk_upload_mapped(
                self.ctx, self._ptr(dev), _u64(np.ascontiguousarray(offs[idx])), srcp,
                _u64(np.ascontiguousarray(staged["disk"][idx])), _u8(flags), len(idx), _u32(st)), "vk_upload_mapped")
            for j, i in enumerate(idx):
                if st[j]:   # the pages could not be registered: through a pageable copy, once
                    dev[int(offs[i]):int(offs[i]) + views[j].size].copy_(torch.from_numpy(views[j].copy()))
            del views, srcp
            self._release_mapped(mapped, idx)
            for i in np.flatnonzero(~is_gz):           # the files that could not be mapped lie in the staging buffer
                if int(i) not in idx and int(staged["disk"][i]):
                    o, nb = int(offs[i]), int(staged["disk"][i])
                    dev[o:o + nb].copy_(pinned[o:o + nb], non_blocking=True)
        else:
            dev = torch.empty(staged["text_total"], dtype=torch.uint8, device=self.device)
            if plain_total:
                dev[:plain_total].copy_(pinned[:plain_total], non_blocking=True)
        gi = np.flatnonzero(is_gz & (staged["disk"] > 0))
        if gi.size:
            # the compressed bytes are not copied: the inflate kernels read them where they are, in the pinned
            # staging buffer, over PCIe (each byte once by the block-start finder and once by the decoder,
            # ~12 GB/s of a 57 GB/s link) -- 27 ms of H2D copy per 1.5 GB that nothing had to wait for
            # ... or, for a rank with few I/O threads, in the files' own page-cache pages (mapped and pinned by stage_files):
            # every file's address, as an offset from the lowest one
            addr = np.array([mapped[int(i)][1].ctypes.data if int(i) in mapped else pinned.data_ptr() + int(staged["src"][i])
                             for i in gi], dtype=np.uint64)
            gzdev = int(addr.min())
            rel = addr - np.uint64(gzdev)
            import time
            ti = time.perf_counter()
            # A BGZF file goes in as its members: no member refers to another, so each is a gzip file of its
            # own -- a wavefront per member instead of one per file, its size and CRC-32 checked like any file's.
            table = staged.get("bgzf") or {}
            go, gl, oo, oc, owner = [], [], [], [], []
            for j, i in enumerate(gi):
                base = rel[j]
                if int(i) in table:
                    mo, ms, mt = table[int(i)]
                    ends = np.cumsum(mt)
                    go.append(base + mo)
                    gl.append(ms)
                    oo.append(offs[i] + ends - mt)
                    oc.append(mt)
                    owner.append(np.full(mo.size, j, dtype=np.int64))
                else:
                    go.append(np.array([base], dtype=np.uint64))
                    gl.append(staged["disk"][i:i + 1])
                    oo.append(offs[i:i + 1])
                    oc.append(staged["caps"][i:i + 1])
                    owner.append(np.array([j], dtype=np.int64))
            owner = np.concatenate(owner)
            g1, s1 = self.inflate(gzdev, np.concatenate(go), np.concatenate(gl), dev, np.concatenate(oo), np.concatenate(oc))
            got = np.zeros(gi.size, dtype=np.uint64)
            st = np.zeros(gi.size, dtype=np.uint32)
            np.add.at(got, owner, g1)
            np.bitwise_or.at(st, owner, s1)
            if timings is not None:
                timings["inflate_s"] = timings.get("inflate_s", 0.0) + time.perf_counter() - ti
            # More text than the slot held (several members and only the last one's size word known, or a
            # file that expands past GZ_MAX_FIRST_RATIO): inflate those again into a side buffer -- of the
            # size the first pass reported where it could (the chunked path decodes the whole file before it
            # looks at the slot), else of 32x, 256x and finally DEFLATE's limit of 1032x the compressed size.
            tried = {j: int(staged["caps"][gi[j]]) for j in range(gi.size)}   # the slot size of each file's last attempt
            for grow in (32, 256, 1032):
                over = [j for j in range(gi.size) if st[j] == _capi.VK_GZ_OVERFLOW]
                if not over:
                    break
                oi = gi[over]
                # (a length beyond the slot is the size the call reported as needed; one within it is what fitted)
                # -- never a slot that is not larger than the one that just overflowed (a small file's first slot,
                # 64x its size, is above the ladder's first steps)
                c2 = np.array([int(got[jj]) if int(got[jj]) > tried[jj] else
                               max(int(staged["disk"][gi[jj]]) * grow + (1 << 16), 2 * tried[jj]) for jj in over], dtype=np.uint64)
                for j, jj in enumerate(over):
                    tried[jj] = int(c2[j])
                o2 = np.zeros(oi.size, dtype=np.uint64)
                p = 0
                for j in range(oi.size):
                    o2[j] = p
                    p += (int(c2[j]) + 15) // 16 * 16
                try:
                    side = torch.empty(p + 16, dtype=torch.uint8, device=self.device)
                except RuntimeError as e:       # no room for that much text: these files fail, the batch lives
                    print("gzip inflate: no memory for", p, "bytes of text:", repr(e)[:120], file=sys.stderr)
                    break
                g2, s2 = self.inflate(gzdev, rel[over], staged["disk"][oi], side, o2, c2)
                base = dev.numel()
                dev = torch.cat([dev, side])
                del side
                for j, jj in enumerate(over):
                    got[jj], st[jj] = g2[j], s2[j]
                    offs = offs.copy() if offs is staged["offs"] else offs
                    offs[oi[j]] = base + int(o2[j])
            for j, i in enumerate(gi):
                if st[j]:
                    print(f"gzip inflate failed (status {int(st[j])}):", staged["paths"][i], file=sys.stderr)
                    fstat[i] = st[j]
                else:
                    lens[i] = got[j]
            if mapped:
                self._release_mapped(mapped)   # (every inflate call has synchronised)
        torch.cuda.current_stream(self.device).synchronize()
        if mapped:
            self._release_mapped(mapped)
        return dev, offs, lens

    def upload_files(self, paths, pool=None):
        """Like upload() for files on disk (stage_files + upload_staged)."""
        return self.upload_staged(self.stage_files(paths, pool))

    def inflate(self, gz, gz_offsets, gz_lengths, out, out_offsets, out_caps):
        """gzip files -> FASTQ text in HBM (vk_inflate_device; dsk reads .gz natively,
        commands/image.py:771-790).  gz: uint8 tensor in device memory or in pinned host memory (the
        kernels read it in place); out: uint8 device tensor; offsets / lengths / caps: uint64 arrays.  Returns (text_lengths uint64[n], status uint32[n] of VK_GZ_* bits); synchronises."""
        n = len(gz_offsets)
        go, gl = self._desc(gz_offsets, gz_lengths)
        oo, oc = self._desc(out_offsets, out_caps)
        lens = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint32)
        gzp = C.c_void_p(gz) if isinstance(gz, int) else self._ptr(gz)   # (an address: host memory pinned for the GPU)
        st = self.L.vk_inflate_device(self.ctx, gzp, _u64(go), _u64(gl), n, self._ptr(out), _u64(oo), _u64(oc), _u64(lens),
                                      _u32(status))
        _capi.check(self.ctx, st, "vk_inflate_device")
        return lens, status

    # -- stages ----------------------------------------------------------------
    def count(self, fastq, offsets, lengths, parts=0, hist=None, status=None):
        """K1 (+check): forward-strand histograms int32/uint32 [n, 4^k] and status [n]."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        if hist is None:
            hist = torch.empty((n, self.ncode), dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.int32, device=self.device)
        st = self.L.vk_count_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), n, self.k, parts, self._ptr(hist),
                                    self._ptr(status))
        _capi.check(self.ctx, st, "vk_count_device")
        return hist, status

    def count_fasta(self, fasta, offsets, lengths, hist=None, status=None, bases=None):
        """FASTA text in HBM (laid out as for count) -> (hist [n, 4^k], status [n], bases int64 [n] = each sample's
        sequence bytes), all on the device (vk_count_fasta_device)."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        if hist is None:
            hist = torch.empty((n, self.ncode), dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.int32, device=self.device)
        if bases is None:
            bases = torch.empty((n,), dtype=torch.int64, device=self.device)
        st = self.L.vk_count_fasta_device(self.ctx, self._ptr(fasta), _u64(offs), _u64(lens), n, self.k, self._ptr(hist),
                                          self._ptr(status), self._ptr(bases))
        _capi.check(self.ctx, st, "vk_count_fasta_device")
        return hist, status, bases

    def count_fasta_sampled(self, fasta, offsets, lengths, frag_len, pair_sample, seeds, thresholds, shifts):
        """The subsample ladder of FASTA samples in HBM (vk_count_fasta_sampled_device; the rule: INTEGRATION.md,
        "--from-fasta --fragments"): pair i counts sample pair_sample[i] over the fragments of frag_len bytes that
        (seeds[i], thresholds[i], shifts[i]) take.  Returns (hist [npairs, 4^k], status [n], bases int64 [n], taken int64
        [npairs] = the sequence bytes in taken fragments), all on the device."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        ps = np.ascontiguousarray(pair_sample, dtype=np.uint32)
        sd, th, sh = (np.ascontiguousarray(a, dtype=np.uint64) for a in (seeds, thresholds, shifts))
        if not (ps.ndim == 1 and ps.shape == sd.shape == th.shape == sh.shape):
            raise ValueError("pair_sample, seeds, thresholds and shifts must be 1-D and of equal length")
        hist = torch.empty((len(ps), self.ncode), dtype=torch.int32, device=self.device)
        status = torch.empty((n,), dtype=torch.int32, device=self.device)
        bases = torch.empty((n,), dtype=torch.int64, device=self.device)
        taken = torch.empty((len(ps),), dtype=torch.int64, device=self.device)
        st = self.L.vk_count_fasta_sampled_device(self.ctx, self._ptr(fasta), _u64(offs), _u64(lens), n, self.k, int(frag_len),
                                                  len(ps), _u32(ps), _u64(sd), _u64(th), _u64(sh), self._ptr(hist),
                                                  self._ptr(status), self._ptr(bases), self._ptr(taken))
        _capi.check(self.ctx, st, "vk_count_fasta_sampled_device")
        return hist, status, bases, taken

    def fasta_records(self, fasta, offsets, lengths):
        """The records of FASTA samples in HBM (vk_fasta_records_count_device, vk_fasta_records_device; the rule:
        INTEGRATION.md, "--from-fasta --per-record"): (rec_first uint64 [n + 1] = prefix sums of the samples' record
        counts, start uint64 [total], bases uint64 [total], names = [bytes] of at most VK_FA_NAME_BYTES, status uint32
        [n]), all on the host; synchronises."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        nrec = torch.zeros((n,), dtype=torch.int32, device=self.device)
        status = torch.zeros((n,), dtype=torch.int32, device=self.device)
        st = self.L.vk_fasta_records_count_device(self.ctx, self._ptr(fasta), _u64(offs), _u64(lens), n, self._ptr(nrec),
                                                  self._ptr(status))
        _capi.check(self.ctx, st, "vk_fasta_records_count_device")
        rec_first = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(nrec.cpu().numpy().view(np.uint32), out=rec_first[1:])
        total = int(rec_first[n])
        start = torch.zeros((max(total, 1),), dtype=torch.int64, device=self.device)
        bases = torch.zeros((max(total, 1),), dtype=torch.int64, device=self.device)
        name = torch.zeros((max(total, 1), _capi.VK_FA_NAME_BYTES), dtype=torch.uint8, device=self.device)
        st = self.L.vk_fasta_records_device(self.ctx, self._ptr(fasta), _u64(offs), _u64(lens), n, _u64(rec_first),
                                            self._ptr(start), self._ptr(bases), self._ptr(name))
        _capi.check(self.ctx, st, "vk_fasta_records_device")
        raw = name.cpu().numpy()[:total]
        names = [bytes(row).rstrip(b"\0") for row in raw]
        return (rec_first, start.cpu().numpy().view(np.uint64)[:total], bases.cpu().numpy().view(np.uint64)[:total], names,
                status.cpu().numpy().view(np.uint32))

    def count_fasta_records(self, fasta, offsets, lengths, rec_first, slot, nslots):
        """One histogram per selected record (vk_count_fasta_records_device): slot uint32 [total] names the row of every
        record of the batch or VK_FA_NO_SLOT.  Returns hist [nslots, 4^k] on the device."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        rec_first = np.ascontiguousarray(rec_first, dtype=np.uint64)
        slot = np.ascontiguousarray(slot, dtype=np.uint32)
        if rec_first.shape != (n + 1,) or slot.shape != (int(rec_first[n]),):
            raise ValueError("rec_first must hold n + 1 prefix sums and slot one entry per record")
        d_slot = torch.from_numpy(slot.view(np.int32) if slot.size else np.zeros(1, dtype=np.int32)).to(self.device)
        hist = torch.empty((int(nslots), self.ncode), dtype=torch.int32, device=self.device)
        st = self.L.vk_count_fasta_records_device(self.ctx, self._ptr(fasta), _u64(offs), _u64(lens), n, self.k, _u64(rec_first),
                                                  self._ptr(d_slot), int(nslots), self._ptr(hist))
        _capi.check(self.ctx, st, "vk_count_fasta_records_device")
        return hist

    def count_fasta_windows(self, fasta, offsets, lengths, rec_first, rec_bases, win_first, win_len, win_step, row_lo, nrows,
                            tile_rows=0, hist=None):
        """One histogram per window of the selected records (vk_count_fasta_windows_device; the rule: INTEGRATION.md,
        "--from-fasta --windows"): rec_bases uint64 [total] as fasta_records gives them, win_first uint64 [total] = the row
        of every record's window 0 or VK_FA_NO_WINDOW (both on the host or already on the device as int64 tensors).  The
        rows of [row_lo, row_lo + nrows) are counted; tile_rows: with win_step < win_len, the tile rows the range needs
        (fasta.window_plan states them).  Returns hist [nrows, 4^k] on the device."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        rec_first = np.ascontiguousarray(rec_first, dtype=np.uint64)
        if rec_first.shape != (n + 1,):
            raise ValueError("rec_first must hold n + 1 prefix sums")
        total = int(rec_first[n])

        def on_device(a, what):
            if not isinstance(a, torch.Tensor):
                a = np.ascontiguousarray(a, dtype=np.uint64)
                a = torch.from_numpy(a.view(np.int64) if a.size else np.zeros(1, dtype=np.int64)).to(self.device)
            if a.dtype != torch.int64 or a.numel() < max(total, 1):
                raise ValueError(f"{what} must hold one 64-bit entry per record")
            return a
        d_bases, d_first = on_device(rec_bases, "rec_bases"), on_device(win_first, "win_first")
        if hist is None:
            hist = torch.empty((int(nrows), self.ncode), dtype=torch.int32, device=self.device)
        st = self.L.vk_count_fasta_windows_device(self.ctx, self._ptr(fasta), _u64(offs), _u64(lens), n, self.k, _u64(rec_first),
                                                  self._ptr(d_bases), self._ptr(d_first), int(win_len), int(win_step), int(row_lo),
                                                  int(nrows), int(tile_rows), self._ptr(hist))
        _capi.check(self.ctx, st, "vk_count_fasta_windows_device")
        return hist

    # -- BAM ---------------------------------------------------------------------
    def _bam_call(self, bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, exclude, flags, groups=None,
                  stream_group=None, out=None, out_offsets=None, out_caps=None):
        """One of the four BAM calls, marshalled and issued: with `groups` a grouped one, with `out` a text call.  A
        framing call returns (records uint64 [nstreams], text bytes uint64 [nstreams], status uint32 [nfiles]), a text
        call (text lengths uint64 [nstreams], status uint32 [nfiles]); on the host, synchronised."""
        offs, lens = self._desc(offsets, lengths)
        first = np.ascontiguousarray(first_record, dtype=np.uint64)
        nref = np.ascontiguousarray(n_ref, dtype=np.int32)
        sf = np.ascontiguousarray(stream_file, dtype=np.uint32)
        sel = np.ascontiguousarray(stream_select, dtype=np.uint32)
        if first.shape != offs.shape or nref.shape != offs.shape or sf.ndim != 1 or sf.shape != sel.shape:
            raise ValueError("first_record and n_ref: one per file; stream_file and stream_select: one per stream")
        args = [self.ctx, self._ptr(bam), _u64(offs), _u64(lens), _u64(first), nref.ctypes.data_as(C.POINTER(C.c_int32)), len(offs)]
        if groups is not None:
            gfirst, ifirst, raw = _bam_group_args(len(offs), groups)
            sg = np.ascontiguousarray(stream_group, dtype=np.uint32)
            if sg.shape != sf.shape:
                raise ValueError("stream_group: one per stream")
            args += [_u32(gfirst), _u32(ifirst), raw.ctypes.data_as(C.POINTER(C.c_uint8)), _u32(sf), _u32(sel), _u32(sg)]
        else:
            args += [_u32(sf), _u32(sel)]
        args += [len(sf), int(exclude), int(flags)]
        status = np.zeros(len(offs), dtype=np.uint32)
        if out is not None:
            oo, oc = self._desc(out_offsets, out_caps)
            if oo.shape != sf.shape:
                raise ValueError("out_offsets and out_caps: one per stream")
            got = np.zeros(len(sf), dtype=np.uint64)
            args += [self._ptr(out), _u64(oo), _u64(oc), _u64(got), _u32(status)]
            res = (got, status)
        else:
            recs = np.zeros(len(sf), dtype=np.uint64)
            nbytes = np.zeros(len(sf), dtype=np.uint64)
            args += [_u64(recs), _u64(nbytes), _u32(status)]
            res = (recs, nbytes, status)
        name = {(False, False): "vk_bam_frame_device", (False, True): "vk_bam_fastq_device",
                (True, False): "vk_bam_groups_frame_device", (True, True): "vk_bam_groups_fastq_device"}[groups is not None, out is not None]
        _capi.check(self.ctx, getattr(self.L, name)(*args), name)
        return res

    def _bam_text(self, frame, fastq, a, exclude, flags):
        """A text buffer sized by the framing call `frame` (every stream at a multiple of 16 bytes, as upload() lays
        samples out) and filled by the text call `fastq`, both on the arguments `a`: (records, out, offsets, lengths,
        status)."""
        recs, nbytes, _ = frame(*a, exclude, flags)
        oo, total = slots16(nbytes)
        torch = _torch()
        out = torch.zeros(total + 16, dtype=torch.uint8, device=self.device)
        got, status = fastq(*a, out, oo, nbytes, exclude, flags)
        return recs, out, oo, got, status

    def bam_frame(self, bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, exclude=0x900, flags=0):
        """The reads of BAM files whose inflated bytes lie in HBM (vk_bam_frame_device; the rule: INTEGRATION.md,
        "--from-bam: the rule"): stream s takes the reads stream_select[s] (VK_BAM_ALL / READ1 / READ2 / SINGLE) of file
        stream_file[s].  Returns (records uint64 [nstreams], text bytes uint64 [nstreams], status uint32 [nfiles] of
        VK_BAM_* bits) on the host; synchronises."""
        return self._bam_call(bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, exclude, flags)

    def bam_fastq(self, bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, out, out_offsets, out_caps,
                  exclude=0x900, flags=0):
        """The FASTQ text of those streams (vk_bam_fastq_device) into `out` (uint8 device tensor) at out_offsets, at most
        out_caps bytes each.  Returns (text lengths uint64 [nstreams], status uint32 [nfiles]) on the host;
        synchronises."""
        return self._bam_call(bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, exclude, flags, out=out,
                              out_offsets=out_offsets, out_caps=out_caps)

    def bam_to_fastq(self, bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, exclude=0x900, flags=0):
        """bam_frame, a text buffer sized by it (every stream at a multiple of 16 bytes, as upload() lays samples out), and
        bam_fastq: (text uint8 device tensor, offsets uint64 [nstreams], lengths uint64 [nstreams], status uint32
        [nfiles]).  `bam` stays the caller's."""
        a = (bam, offsets, lengths, first_record, n_ref, stream_file, stream_select)
        _, out, oo, got, status = self._bam_text(self.bam_frame, self.bam_fastq, a, exclude, flags)
        return out, oo, got, status

    def last_bam_frame(self):
        """(segments, segments walked again) of the last bam_frame / bam_fastq call (vk_last_bam_frame)."""
        seg, re = C.c_uint64(), C.c_uint64()
        _capi.check(self.ctx, self.L.vk_last_bam_frame(self.ctx, C.byref(seg), C.byref(re)), "vk_last_bam_frame")
        return seg.value, re.value

    # -- BAM, split by read group ---------------------------------------------------
    def bam_groups_frame(self, bam, offsets, lengths, first_record, n_ref, groups, stream_file, stream_select, stream_group,
                         exclude=0x900, flags=0):
        """bam_frame with the reads split by read group (vk_bam_groups_frame_device; the rule: INTEGRATION.md, "--from-bam
        --bam-read-groups: the rule"): groups[i] = the IDs (bytes) of file i's @RG lines, stream s takes the reads
        stream_select[s] of group stream_group[s] (an index into groups[stream_file[s]], or VK_BAM_UNGROUPED) of file
        stream_file[s].  Returns (records uint64 [nstreams], text bytes uint64 [nstreams], status uint32 [nfiles]: VK_BAM_*,
        VK_BAM_BAD_AUX among them) on the host; synchronises."""
        return self._bam_call(bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, exclude, flags, groups=groups,
                              stream_group=stream_group)

    def bam_groups_fastq(self, bam, offsets, lengths, first_record, n_ref, groups, stream_file, stream_select, stream_group, out,
                         out_offsets, out_caps, exclude=0x900, flags=0):
        """The FASTQ text of those streams (vk_bam_groups_fastq_device) into `out` (uint8 device tensor) at out_offsets, at
        most out_caps bytes each.  Returns (text lengths uint64 [nstreams], status uint32 [nfiles]) on the host;
        synchronises."""
        return self._bam_call(bam, offsets, lengths, first_record, n_ref, stream_file, stream_select, exclude, flags, groups=groups,
                              stream_group=stream_group, out=out, out_offsets=out_offsets, out_caps=out_caps)

    def bam_groups_to_fastq(self, bam, offsets, lengths, first_record, n_ref, groups, stream_file, stream_select, stream_group,
                            exclude=0x900, flags=0):
        """bam_groups_frame, a text buffer sized by it (every stream at a multiple of 16 bytes) and bam_groups_fastq: (text
        uint8 device tensor, offsets uint64 [nstreams], lengths uint64 [nstreams], reads uint64 [nstreams], status uint32
        [nfiles]).  `bam` stays the caller's."""
        a = (bam, offsets, lengths, first_record, n_ref, groups, stream_file, stream_select, stream_group)
        recs, out, oo, got, status = self._bam_text(self.bam_groups_frame, self.bam_groups_fastq, a, exclude, flags)
        return out, oo, got, recs, status

    def bam_groups_workspace_size(self, lengths, groups, stream_file, seg_bytes=0, panel_segs=0):
        """Bytes of workspace the grouped calls take beyond the ungrouped ones (vk_bam_groups_workspace_size; host only)."""
        return bam_groups_workspace_size(lengths, groups, stream_file, seg_bytes, panel_segs, self.L)

    def last_bam_groups(self):
        """(workgroups of the emit launch, records whose aux was walked) of the last bam_groups_frame / bam_groups_fastq
        call (vk_last_bam_groups)."""
        wgs, walked = C.c_uint64(), C.c_uint64()
        _capi.check(self.ctx, self.L.vk_last_bam_groups(self.ctx, C.byref(wgs), C.byref(walked)), "vk_last_bam_groups")
        return wgs.value, walked.value

    def count_sampled(self, fastq, offsets, lengths, seeds, thresholds, parts=0, hist=None, status=None,
                      sites=None):
        """K1 over a pseudo-random subset of each sample's reads (vk_count_sampled_device):
        seeds / thresholds are per-sample host arrays (threshold = fraction * 2^32, 2^32 = all).
        Returns (hist [n, 4^k], status [n], sites int64 [n, 2] = (bytes of all sequence lines,
        bytes of the sequence lines of the reads taken))."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (n,)))
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.uint64), (n,)))
        if hist is None:
            hist = torch.empty((n, self.ncode), dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.int32, device=self.device)
        if sites is None:
            sites = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        st = self.L.vk_count_sampled_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), n, self.k, parts, _u64(seeds),
                                            _u64(thr), self._ptr(hist), self._ptr(status), self._ptr(sites))
        _capi.check(self.ctx, st, "vk_count_sampled_device")
        return hist, status, sites

    def read_index(self, fastq, offsets, lengths, parts=0):
        """The read index of a batch (vk_read_index_device): (nsites uint64[n], status uint32[n]) on the host; the
        context keeps the index, and count_sampled calls on these samples walk the reads they take."""
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        sites = np.zeros(n, dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint32)
        st = self.L.vk_read_index_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), n, parts, _u64(sites),
                                         _u32(status))
        _capi.check(self.ctx, st, "vk_read_index_device")
        return sites, status

    def count_index(self, fastq, offsets, lengths, parts=0, hist=None, status=None):
        """count() and read_index() in one pass over the text (vk_count_index_device):
        (hist [n, 4^k] on the device, nsites uint64[n], status uint32[n] on the host)."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        if hist is None:
            hist = torch.empty((n, self.ncode), dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.int32, device=self.device)
        sites = np.zeros(n, dtype=np.uint64)
        st_h = np.zeros(n, dtype=np.uint32)
        st = self.L.vk_count_index_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), n, self.k, parts, self._ptr(hist),
                                          self._ptr(status), _u64(sites), _u32(st_h))
        _capi.check(self.ctx, st, "vk_count_index_device")
        return hist, sites, st_h

    def clean_lines(self, fastq, offsets, lengths):
        """Newline bytes of each file in HBM (vk_clean_lines_device; // 4 = its records).  Synchronises."""
        offs, lens = self._desc(offsets, lengths)
        lines = np.zeros(len(offs), dtype=np.uint64)
        st = self.L.vk_clean_lines_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), len(offs), _u64(lines))
        _capi.check(self.ctx, st, "vk_clean_lines_device")
        return lines

    def clean_heads(self, fastq, offsets, lengths, sample_size=10000):
        """(totals, counted) uint64 per file in HBM: the `total` and `n` of rawinput.avg_read_length over the file's
        first `sample_size` records (vk_clean_heads_device).  One call and one synchronisation for the batch."""
        offs, lens = self._desc(offsets, lengths)
        totals = np.zeros(len(offs), dtype=np.uint64)
        counted = np.zeros(len(offs), dtype=np.uint64)
        st = self.L.vk_clean_heads_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), len(offs), int(sample_size),
                                          _u64(totals), _u64(counted))
        _capi.check(self.ctx, st, "vk_clean_heads_device")
        return totals, counted

    def _workspace(self, size_fn, *args):
        """A workspace tensor of the size that `size_fn` (a vk_*_workspace_size) states for `args`, of 256 bytes at least."""
        ws_bytes = C.c_uint64()
        _capi.check(self.ctx, size_fn(*args, C.byref(ws_bytes)), size_fn.__name__)
        torch = _torch()
        return torch.empty(max(int(ws_bytes.value), 256), dtype=torch.uint8, device=self.device)

    def _records(self, text, offs, lens, records, one_each=None):
        """The samples' record counts in the C ABI's type: the caller's or, with None, every record of the text (clean_lines
        here).  one_each: the caller's message when they are not one per sample (None: not checked)."""
        if records is None:
            records = (self.clean_lines(text, offs, lens) + np.uint64(1)) // np.uint64(4)
        recs = np.ascontiguousarray(records, dtype=np.uint64)
        if one_each is not None and len(recs) != len(offs):
            raise ValueError(one_each)
        return recs

    def _clean_call(self, offsets, lengths, records, roles, samples, nsamples, size_fn):
        """What clean() and detect_adapters() do alike ahead of their call: the files' arrays in the C ABI's types, with
        their count, and a workspace tensor of the size `size_fn` (vk_clean_workspace_size or its detect twin) asks."""
        offs, lens = self._desc(offsets, lengths)
        recs = np.ascontiguousarray(records, dtype=np.uint64)
        roles = np.ascontiguousarray(roles, dtype=np.uint32)
        samples = np.ascontiguousarray(samples, dtype=np.uint32)
        n = len(offs)
        if not (len(recs) == len(roles) == len(samples) == n):
            raise ValueError("one record budget, role and sample per file")
        return offs, lens, recs, roles, samples, n, self._workspace(size_fn, _u64(lens), _u64(recs), n, nsamples)

    def detect_adapters(self, fastq, offsets, lengths, records, roles, samples, nsamples, trim_tail=10):
        """Each group's adapter detected from its first reads (vk_clean_detect_device; the files, records, roles and
        samples of clean()): a list of [R1's, R2's, the single reads'] per sample, bytes or None.  Synchronises."""
        offs, lens, recs, roles, samples, n, ws = self._clean_call(offsets, lengths, records, roles, samples, nsamples,
                                                                   self.L.vk_clean_detect_workspace_size)
        alen = np.zeros(3 * nsamples, dtype=np.uint32)
        aseq = np.zeros((3 * nsamples, _capi.VK_CL_MAX_ADAPTER), dtype=np.uint8)
        st = self.L.vk_clean_detect_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), _u64(recs), _u32(roles),
                                           _u32(samples), n, nsamples, int(trim_tail), self._ptr(ws), ws.numel(), _u32(alen),
                                           _u8(aseq))
        _capi.check(self.ctx, st, "vk_clean_detect_device")
        return [[aseq[3 * j + g, :alen[3 * j + g]].tobytes() if alen[3 * j + g] else None for g in range(3)]
                for j in range(nsamples)]

    def clean(self, fastq, offsets, lengths, records, roles, samples, nsamples, trim=(10, 10), adapter=True, merge=True,
              dedup=True, adapters=None):
        """Step B for a batch of samples whose raw files are in HBM (vk_clean_device): file i gives its first
        records[i] records to sample samples[i] as roles[i] (_capi.VK_CL_ROLE_*).  Returns (text uint8 tensor on the
        device, offsets uint64[nsamples], lengths uint64[nsamples], stats uint64[nsamples, VK_CL_NSTAT], status
        uint32[nsamples]); the arrays on the host (the call waits for the kernels).

        adapters: per sample [R1's, R2's, the single reads'] adapter (bytes or None) to trim by sequence as well
        (vk_clean_adapters_device); the result then ends with adapter stats uint64[nsamples, 2] (reads, bases cut)."""
        torch = _torch()
        offs, lens, recs, roles, samples, n, ws = self._clean_call(offsets, lengths, records, roles, samples, nsamples,
                                                                   self.L.vk_clean_workspace_size)
        cap = np.zeros(nsamples, dtype=np.uint64)
        np.add.at(cap, samples.astype(np.int64), lens)
        out_offs, total = slots16(cap)
        total += 16
        out = torch.empty(total, dtype=torch.uint8, device=self.device)
        out_lens = torch.empty(nsamples, dtype=torch.int64, device=self.device)
        stats = torch.empty((nsamples, _capi.VK_CL_NSTAT), dtype=torch.int64, device=self.device)
        status = torch.empty(nsamples, dtype=torch.int32, device=self.device)
        results = [(out_lens, np.uint64), (stats, np.uint64), (status, np.uint32)]   # (device tensor, its type on the host)
        flags = (_capi.VK_CL_ADAPTER if adapter else 0) | (_capi.VK_CL_MERGE if merge else 0) | (_capi.VK_CL_DEDUP if dedup else 0)
        args = (self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), _u64(recs), _u32(roles), _u32(samples), n, nsamples,
                int(trim[0]), int(trim[1]), flags, self._ptr(ws), ws.numel(), self._ptr(out), _u64(out_offs), total,
                self._ptr(out_lens), self._ptr(stats), self._ptr(status))
        if adapters is None:
            _capi.check(self.ctx, self.L.vk_clean_device(*args), "vk_clean_device")
        else:
            if len(adapters) != nsamples:
                raise ValueError("one adapter triple per sample")
            alen = np.zeros(3 * nsamples, dtype=np.uint32)
            aseq = np.zeros((3 * nsamples, _capi.VK_CL_MAX_ADAPTER), dtype=np.uint8)
            for j, triple in enumerate(adapters):
                for g, a in enumerate(triple):
                    if a is None:
                        continue
                    if not 0 < len(a) <= _capi.VK_CL_MAX_ADAPTER:
                        raise ValueError(f"an adapter is 1..{_capi.VK_CL_MAX_ADAPTER} bytes: {a!r}")
                    alen[3 * j + g] = len(a)
                    aseq[3 * j + g, :len(a)] = np.frombuffer(bytes(a), dtype=np.uint8)
            ad_stats = torch.empty((nsamples, 2), dtype=torch.int64, device=self.device)
            results.append((ad_stats, np.uint64))
            st = self.L.vk_clean_adapters_device(*args, _u32(alen), _u8(aseq), self._ptr(ad_stats))
            _capi.check(self.ctx, st, "vk_clean_adapters_device")
        return (out, out_offs) + tuple(t.cpu().numpy().astype(dt) for t, dt in results)

    def ladder_emit(self, fastq, offsets, lengths, step_sample, step_seed, step_threshold, step_whole, records=None,
                    capacity=None, out=None):
        """Step C's files for cleaned samples in HBM (vk_ladder_emit_device): step j writes the reads of sample
        step_sample[j] that count_sampled counts with step_seed[j] / step_threshold[j] -- with step_whole[j] every
        read, as count does -- as FASTQ text.  records: the samples' record counts (None: clean_lines here).
        Returns (text uint8 tensor on the device, offsets uint64[nsteps], lengths uint64[nsteps], status
        uint32[nsamples]); a sample with a non-zero status gives no text.  capacity: bytes of the text buffer (None:
        what the selection is expected to take; the call is repeated once with the size it reports when that falls
        short); with a capacity given, text that does not fit raises VkError(VK_ENOSPC) and nothing is written.  out: the
        text buffer to use (a uint8 device tensor of at least `capacity` bytes).  Synchronises."""
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        sidx = np.ascontiguousarray(step_sample, dtype=np.uint32)
        seeds = np.ascontiguousarray(step_seed, dtype=np.uint64)
        thr = np.ascontiguousarray(step_threshold, dtype=np.uint64)
        whole = np.ascontiguousarray(step_whole, dtype=np.uint8)
        ns = len(sidx)
        if not (len(seeds) == len(thr) == len(whole) == ns):
            raise ValueError("one sample, seed, threshold and whole flag per step")
        recs = self._records(fastq, offs, lens, records)
        ws = self._workspace(self.L.vk_ladder_emit_workspace_size, _u64(recs), n, _u64(lens), _u32(sidx), ns)
        out_offs = np.zeros(ns, dtype=np.uint64)
        out_lens = np.zeros(ns, dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint32)
        if out is not None and (capacity is None or out.numel() < capacity):
            raise ValueError("a text buffer needs its capacity, within its size")
        want = capacity
        if want is None:   # (a read's text is its record's, and a cut read's header comes once per piece: a tenth on top)
            share = np.where(whole != 0, 1.0, thr.astype(np.float64) / float(1 << 32))
            want = int((share * lens[sidx.astype(np.int64)].astype(np.float64)).sum() * 1.1) + 16 * ns + 4096
        for attempt in range(2):
            if out is None or capacity is None:
                out = torch.empty(want + 64, dtype=torch.uint8, device=self.device)   # (readable past the last file's end)
            st = self.L.vk_ladder_emit_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), _u64(recs), n, _u32(sidx),
                                              _u64(seeds), _u64(thr), _u8(whole), ns, self._ptr(out), want, _u64(out_offs),
                                              _u64(out_lens), _u32(status), self._ptr(ws), ws.numel())
            if st != _capi.VK_ENOSPC or capacity is not None or attempt:
                break
            out = None   # (free the short buffer before the next one is made)
            want = int(((out_lens + np.uint64(15)) // np.uint64(16) * np.uint64(16)).sum())
        _capi.check(self.ctx, st, "vk_ladder_emit_device")
        return out, out_offs, out_lens, status

    def screen_set(self, fasta, length, k=31, slots=None):
        """The k-mer set of a reference FASTA whose text lies in HBM (vk_screen_build_device; the rule: INTEGRATION.md,
        "--exclude-fasta / --keep-fasta: the rule"): fasta a uint8 device tensor readable up to the 16-byte rounded end of
        its first `length` bytes, k in 16..31.  slots: the table's size, a power of two of at least 1,024 (None: the
        smallest that is at least twice the number of windows).  Returns a ScreenSet (table, slots, k, distinct,
        windows); a text that does not begin with '>' raises ValueError.  Synchronises."""
        torch = _torch()
        length = int(length)
        if not _capi.VK_SCREEN_MIN_K <= int(k) <= _capi.VK_SCREEN_MAX_K:
            raise ValueError(f"the screen's k is {_capi.VK_SCREEN_MIN_K}..{_capi.VK_SCREEN_MAX_K}: {k}")
        if length > _capi.VK_SCREEN_MAX_REF:   # (before anything is allocated)
            raise ValueError(f"a screen reference holds at most 2^30 sequence bytes: {length} bytes of text")
        ws = self._workspace(self.L.vk_screen_build_workspace_size, length)
        windows, distinct, status = C.c_uint64(), C.c_uint64(), C.c_uint32()

        def call(table, n):
            st = self.L.vk_screen_build_device(self.ctx, self._ptr(fasta), length, int(k), self._ptr(table) if n else None, n,
                                               self._ptr(ws), ws.numel(), C.byref(windows), C.byref(distinct), C.byref(status))
            _capi.check(self.ctx, st, "vk_screen_build_device")
            if status.value:
                raise ValueError("the screen's reference is no FASTA text: it does not begin with '>'")

        if slots is None:
            call(None, 0)
            slots = _capi.VK_SCREEN_MIN_SLOTS
            while slots < 2 * windows.value:
                slots *= 2
        table = torch.empty(int(slots), dtype=torch.int64, device=self.device)
        call(table, int(slots))
        return ScreenSet(table, int(slots), int(k), int(distinct.value), int(windows.value))

    def screen(self, text, offs, lens, sset, keep=False, min_hits=1, records=None):
        """Cleaned samples in HBM screened record by record against a ScreenSet (vk_screen_device): keep=False keeps the
        records with fewer than min_hits window positions in the set (--exclude-fasta), keep=True the others
        (--keep-fasta).  records: the samples' record counts (None: clean_lines here).  Returns (out uint8 device tensor,
        out_offs uint64[n], out_lens uint64[n], stats uint64[n, 4] = records in, records kept, sequence bases in,
        sequence bases kept, status uint32[n]); sample i's text is out[out_offs[i] .. + out_lens[i]), laid out as clean()
        lays its output out; a sample with a status gets no text.  Synchronises."""
        torch = _torch()
        offs, lens = self._desc(offs, lens)
        n = len(offs)
        if int(min_hits) < 1:
            raise ValueError("min_hits is at least 1")
        recs = self._records(text, offs, lens, records, "one record count per sample")
        ws = self._workspace(self.L.vk_screen_workspace_size, _u64(recs), n, _u64(lens))
        out_offs, total = slots16(lens)
        total += 16
        out = torch.empty(total, dtype=torch.uint8, device=self.device)
        out_lens = torch.empty(n, dtype=torch.int64, device=self.device)
        stats = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        st = self.L.vk_screen_device(self.ctx, self._ptr(text), _u64(offs), _u64(lens), _u64(recs), n, self._ptr(sset.table),
                                     sset.slots, sset.k, int(min_hits), 1 if keep else 0, self._ptr(out), _u64(out_offs), total,
                                     self._ptr(out_lens), self._ptr(stats), self._ptr(status), self._ptr(ws), ws.numel())
        _capi.check(self.ctx, st, "vk_screen_device")
        # (the copies below wait for the kernels: the workspace is free after them)
        return (out, out_offs, out_lens.cpu().numpy().astype(np.uint64), stats.cpu().numpy().astype(np.uint64),
                status.cpu().numpy().astype(np.uint32))

    def qc(self, text, offs, lens, records=None):
        """The quality profiles of FASTQ streams in HBM, raw or cleaned (vk_qc_device; the rule: INTEGRATION.md,
        "--qc-report: the rule"): stream i is text[offs[i] .. + lens[i]) and its first records[i] records count (None:
        all of them, by clean_lines here).  Returns (rows uint64[n, VK_QC_NSTAT], status uint32[n]); a stream with a
        status has an all-zero row.  Synchronises."""
        torch = _torch()
        offs, lens = self._desc(offs, lens)
        n = len(offs)
        if n == 0:
            return np.zeros((0, _capi.VK_QC_NSTAT), dtype=np.uint64), np.zeros(0, dtype=np.uint32)
        recs = self._records(text, offs, lens, records, "one record budget per stream")
        ws = self._workspace(self.L.vk_qc_workspace_size, _u64(recs), _u64(lens), n)
        rows = torch.empty((n, _capi.VK_QC_NSTAT), dtype=torch.int64, device=self.device)
        status = torch.empty(n, dtype=torch.int32, device=self.device)
        st = self.L.vk_qc_device(self.ctx, self._ptr(text), _u64(offs), _u64(lens), _u64(recs), n, self._ptr(rows),
                                 self._ptr(status), self._ptr(ws), ws.numel())
        _capi.check(self.ctx, st, "vk_qc_device")
        # (the copies below wait for the kernels: the workspace is free after them)
        return rows.cpu().numpy().view(np.uint64), status.cpu().numpy().astype(np.uint32)

    @staticmethod
    def spectrum_slots(length, every=1):
        """The table of a sample of `length` bytes of FASTQ text: the smallest power of two that is at least max(1024,
        2 ceil(length / 2 / every)).  A record's sequence is less than half its bytes, so at every = 1 the load stays
        below a half and the table cannot fill."""
        want = max(_capi.VK_SCREEN_MIN_SLOTS, 2 * -(-int(length) // (2 * int(every))))
        return 1 << (want - 1).bit_length()

    def _table_group(self, todo, want, table_bytes):
        """The next group of spectrum() and spectrum_fasta(), taken off the front of `todo`: samples in order while their
        tables of want[i] slots fit under table_bytes at 12 bytes a slot (the first always), and the group's tables.
        Returns (group, its indices as an array, nslots, slot bases, keys int64 and counts int32 device tensors)."""
        torch = _torch()
        group, total = [], 0
        while todo and (not group or total + want[todo[0]] * 12 <= int(table_bytes)):
            total += want[todo[0]] * 12
            group.append(todo.pop(0))
        g = np.asarray(group, dtype=np.int64)
        nsl = np.asarray([want[i] for i in group], dtype=np.uint64)
        base = np.zeros(len(group), dtype=np.uint64)
        base[1:] = np.cumsum(nsl[:-1])
        try:
            keys = torch.empty(int(nsl.sum()), dtype=torch.int64, device=self.device)
            counts = torch.empty(int(nsl.sum()), dtype=torch.int32, device=self.device)
        except RuntimeError as e:   # (torch.cuda.OutOfMemoryError is one)
            raise MemoryError(f"no memory for a k-mer table of {int(nsl.sum())} slots ({int(nsl.sum()) * 12} bytes): "
                              "count a sample of the keys with a larger --spectrum-every") from e
        return group, g, nsl, base, keys, counts

    def _spectrum_results(self, n, k, every, sketch):
        """What spectrum() and spectrum_fasta() check and make alike ahead of their groups: k and every, the rows and status
        of n samples and, with sketch=(s, m), the sketches' arrays.  Returns (k, every, rows, status, sk) with sk None or
        (s, m, hashes, info)."""
        k, every = int(k), int(every)
        if not _capi.VK_SCREEN_MIN_K <= k <= _capi.VK_SCREEN_MAX_K:
            raise ValueError(f"the spectrum's k is {_capi.VK_SCREEN_MIN_K}..{_capi.VK_SCREEN_MAX_K}: {k}")
        if every < 1:
            raise ValueError("every is at least 1")
        rows = np.zeros((n, _capi.VK_SPEC_NSTAT), dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint32)
        sk = None
        if sketch is not None:
            sk_s, sk_m = self._sketch_args(*sketch)
            sk = (sk_s, sk_m, np.full((n, sk_s), np.uint64(2 ** 64 - 1), dtype=np.uint64), np.zeros((n, 2), dtype=np.uint64))
        return k, every, rows, status, sk

    def _spectrum_groups(self, lens, every, slots, slots_rule, table_bytes, count, rows, status, sk, depth_step=None):
        """The loop of spectrum() and spectrum_fasta() over their groups: a group's tables (_table_group), the call
        (count(g, keys, counts, base, nsl, d_rows, d_status) returns the workspace it made, kept until the kernels are
        waited for), the sketches while the tables lie there, the rows and status copied back, the depth step
        (depth_step(group, g, keys, counts, base, nsl, d_status)), and the samples whose table filled queued again with four
        times the slots.  slots_rule: spectrum_slots or spectrum_fasta_slots."""
        torch = _torch()
        n = len(lens)
        if slots is None:
            want = [slots_rule(x, every) for x in lens]
            most = [slots_rule(x, 1) for x in lens]
        else:
            want = most = [int(slots)] * n
        todo = list(range(n))
        while todo:
            group, g, nsl, base, keys, counts = self._table_group(todo, want, table_bytes)
            d_rows = torch.empty((len(group), _capi.VK_SPEC_NSTAT), dtype=torch.int64, device=self.device)
            d_status = torch.empty(len(group), dtype=torch.int32, device=self.device)
            ws = count(g, keys, counts, base, nsl, d_rows, d_status)
            # (the copies below wait for the kernels: the tables and the workspace are free after them)
            if sk is not None:   # (while the tables lie there)
                sk[2][g], sk[3][g] = self.sketch_tables(keys, counts, base, nsl, d_status, sk[0], sk[1])
            rows[g] = d_rows.cpu().numpy().view(np.uint64)
            status[g] = d_status.cpu().numpy().astype(np.uint32)
            if depth_step is not None:   # (while the tables lie there; the bands from the rows just read)
                depth_step(group, g, keys, counts, base, nsl, d_status)
            del keys, counts, ws
            # a table that filled (every > 1: the taken keys were more than their expected share): again with four times
            # the slots -- a bounded loop over a status; at slots_rule(., 1) it cannot fill
            again = [i for i in group if status[i] == _capi.VK_SPEC_TABLE_FULL and want[i] < most[i]]
            for i in again:
                want[i] = min(4 * want[i], most[i])
            todo = again + todo

    def spectrum(self, text, offs, lens, k=21, every=1, records=None, slots=None, table_bytes=16 << 30, sketch=None, depth=None):
        """The k-mer spectra of cleaned samples in HBM (vk_spectrum_device; the rule: INTEGRATION.md, "`--kmer-spectrum`:
        the rule"): sample i is text[offs[i] .. + lens[i]), k in 16..31, a key is taken when the high half of its mix is
        a multiple of `every`.  records: the samples' record counts (None: clean_lines here).  Returns (rows
        uint64[n, VK_SPEC_NSTAT], status uint32[n]); a sample with a status has an all-zero row.

        slots=None: sample i's table has spectrum_slots(lens[i], every) slots; with every > 1 a sample that comes back
        VK_SPEC_TABLE_FULL is counted again with four times the slots, up to spectrum_slots(lens[i], 1), where it
        cannot happen.  slots=int forces every sample's table (tests).  The samples are counted in groups whose tables
        together stay under table_bytes at 12 bytes a slot; a sample whose table alone is larger gets a group of its own.

        sketch=(s, m): also the samples' bottom-s MinHash sketches over the keys of multiplicity m and more (sketch_tables;
        the rule: INTEGRATION.md, "`--spectrum-sketch` and `distance`: the rule"), taken from each group's tables before
        they are freed -- a sample counted again from the attempt that succeeded.  Returns (rows, status, hashes
        uint64[n, s], info uint64[n, 2] = eligible, length) then.

        depth: also the samples' reads filtered by their median k-mer depth (depth_filter; the rule: INTEGRATION.md,
        "`--depth-filter`: the rule") against each group's tables before they are freed -- a sample counted again from the
        attempt that succeeded.  One band for every sample or a list of one per sample; a band is a depth.Band or its
        text (resolved per sample from the row's estimates: depth.resolve) or a pair of integers (lo, hi).  The return
        value then also carries (out uint8 device tensor, out_offs uint64[n], out_lens uint64[n], depth_rows
        uint64[n, VK_DEPTH_NSTAT], bands = per sample (lo, hi, applied, reason)); sample i's kept text is out[out_offs[i]
        .. + out_lens[i]), laid out as screen() lays its output out; a sample with a status gets no text and a zero row.
        The spectrum and the sketch describe the text before the filter.  Synchronises."""
        torch = _torch()
        offs, lens = self._desc(offs, lens)
        n = len(offs)
        k, every, rows, status, sk = self._spectrum_results(n, k, every, sketch)
        ret = lambda: (rows, status) + (() if sk is None else sk[2:]) + (() if depth is None else dp)   # noqa: E731
        if depth is not None:
            from . import depth as depth_rules
            from . import spectrum as spectrum_rules
            asked = list(depth) if isinstance(depth, list) else [depth] * n
            if len(asked) != n:
                raise ValueError("one band per sample")
            asked = [depth_rules.parse_band(b) if isinstance(b, str) else b for b in asked]
            out_offs, total = slots16(lens)
            # (one text for all n samples, allocated once: a group writes its samples' regions)
            out = torch.empty(total + 16, dtype=torch.uint8, device=self.device)
            out_lens = np.zeros(n, dtype=np.uint64)
            depth_rows = np.zeros((n, _capi.VK_DEPTH_NSTAT), dtype=np.uint64)
            bands = [None] * n
            dp = (out, out_offs, out_lens, depth_rows, bands)
        if n == 0:
            return ret()
        recs = self._records(text, offs, lens, records, "one record count per sample")

        def count(g, keys, counts, base, nsl, d_rows, d_status):
            o, l, r = offs[g].copy(), lens[g].copy(), recs[g].copy()
            ws = self._workspace(self.L.vk_spectrum_workspace_size, _u64(r), len(g), _u64(l))
            st = self.L.vk_spectrum_device(self.ctx, self._ptr(text), _u64(o), _u64(l), _u64(r), len(g), k, every,
                                           self._ptr(keys), self._ptr(counts), _u64(base), _u64(nsl), self._ptr(d_rows),
                                           self._ptr(d_status), self._ptr(ws), ws.numel())
            _capi.check(self.ctx, st, "vk_spectrum_device")
            return ws

        def depth_step(group, g, keys, counts, base, nsl, d_status):
            for i in group:
                b = asked[i]
                bands[i] = (depth_rules.resolve(b, spectrum_rules.estimate(rows[i], k, every))
                            if isinstance(b, depth_rules.Band) else (int(b[0]), int(b[1]), True, None))
            out_lens[g], depth_rows[g], _ = self.depth_filter(text, offs[g].copy(), lens[g].copy(), keys, counts, base, nsl,
                                                              d_status, [bands[i][0] for i in group],
                                                              [bands[i][1] for i in group], k, every, recs[g].copy(), out,
                                                              out_offs[g].copy())

        self._spectrum_groups(lens, every, slots, self.spectrum_slots, table_bytes, count, rows, status, sk,
                              depth_step if depth is not None else None)
        return ret()

    @staticmethod
    def spectrum_fasta_slots(length, every=1):
        """The table of an assembly of `length` bytes of FASTA text: the smallest power of two that is at least max(1024,
        2 ceil(length / every)).  Windows cannot exceed bytes, so at every = 1 the load stays at a half or below and the
        table cannot fill."""
        want = max(_capi.VK_SCREEN_MIN_SLOTS, 2 * -(-int(length) // int(every)))
        return 1 << (want - 1).bit_length()

    def spectrum_fasta(self, fasta, offs, lens, k=21, every=1, slots=None, table_bytes=16 << 30, sketch=None):
        """The k-mer spectra of assemblies whose FASTA text lies in HBM, laid out as for count_fasta
        (vk_spectrum_fasta_device; the rule: INTEGRATION.md, "`--genome-spectrum`: the rule"): k in 16..31, a key is taken
        when the high half of its mix is a multiple of `every`.  Returns (rows uint64[n, VK_SPEC_NSTAT], status
        uint32[n]): a row is records, bases, windows, taken windows, distinct, hist[256]; a sample with a status has an
        all-zero row.

        slots=None: sample i's table has spectrum_fasta_slots(lens[i], every) slots; with every > 1 a sample that comes
        back VK_SPEC_TABLE_FULL is counted again with four times the slots, up to spectrum_fasta_slots(lens[i], 1), where
        it cannot happen.  slots=int forces every sample's table (tests).  The samples are counted in groups whose tables
        together stay under table_bytes at 12 bytes a slot; a sample whose table alone is larger gets a group of its own.

        sketch=(s, 1): also the samples' bottom-s MinHash sketches (sketch_tables), taken from each group's tables before
        they are freed -- a sample counted again from the attempt that succeeded.  Returns (rows, status, hashes
        uint64[n, s], info uint64[n, 2] = eligible, length) then.  Synchronises."""
        offs, lens = self._desc(offs, lens)
        n = len(offs)
        k, every, rows, status, sk = self._spectrum_results(n, k, every, sketch)
        if sk is not None and sk[1] != 1:
            raise ValueError("an assembly's sketch takes every k-mer: its minimum multiplicity is 1")
        if n == 0:
            return (rows, status) + (() if sk is None else sk[2:])

        def count(g, keys, counts, base, nsl, d_rows, d_status):
            o, l = offs[g].copy(), lens[g].copy()
            ws = self._workspace(self.L.vk_spectrum_fasta_workspace_size, _u64(l), len(g))
            st = self.L.vk_spectrum_fasta_device(self.ctx, self._ptr(fasta), _u64(o), _u64(l), len(g), k, every,
                                                 self._ptr(keys), self._ptr(counts), _u64(base), _u64(nsl), self._ptr(d_rows),
                                                 self._ptr(d_status), self._ptr(ws), ws.numel())
            _capi.check(self.ctx, st, "vk_spectrum_fasta_device")
            return ws

        self._spectrum_groups(lens, every, slots, self.spectrum_fasta_slots, table_bytes, count, rows, status, sk)
        return (rows, status) + (() if sk is None else sk[2:])

    def depth_filter(self, text, offs, lens, keys, counts, base, nslots, table_status, lo, hi, k, every, records, out, out_offs):
        """Cleaned samples in HBM filtered record by record by their median k-mer depth in counting tables that lie in HBM
        (vk_depth_device; the rule: INTEGRATION.md, "`--depth-filter`: the rule"): the samples, k, every and records as
        spectrum() counted them, keys / counts / base / nslots / table_status (an int32 device tensor [n]) as
        vk_spectrum_device left them, lo and hi the samples' bands (integers, both ends included).  Sample i's kept text
        goes to out[out_offs[i] ..), a region of lens[i] rounded up to 16 bytes.  Returns (out_lens uint64[n], rows
        uint64[n, VK_DEPTH_NSTAT], status uint32[n]).  Synchronises."""
        torch = _torch()
        offs, lens = self._desc(offs, lens)
        n = len(offs)
        recs = np.ascontiguousarray(records, dtype=np.uint64)
        base = np.ascontiguousarray(base, dtype=np.uint64)
        nslots = np.ascontiguousarray(nslots, dtype=np.uint64)
        out_offs = np.ascontiguousarray(out_offs, dtype=np.uint64)
        lo = np.ascontiguousarray(lo, dtype=np.uint32)
        hi = np.ascontiguousarray(hi, dtype=np.uint32)
        if not (len(recs) == len(base) == len(nslots) == len(out_offs) == len(lo) == len(hi) == n) or int(table_status.numel()) != n:
            raise ValueError("one record count, base, slot count, status, band and output offset per sample")
        if n and int((base + nslots).max()) > min(int(keys.numel()), int(counts.numel())):
            raise ValueError("a sample's slots lie past the tables")
        ws = self._workspace(self.L.vk_depth_workspace_size, _u64(recs), n, _u64(lens))
        d_lens = torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        d_rows = torch.empty((max(n, 1), _capi.VK_DEPTH_NSTAT), dtype=torch.int64, device=self.device)
        d_status = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        st = self.L.vk_depth_device(self.ctx, self._ptr(text), _u64(offs), _u64(lens), _u64(recs), n, int(k), int(every),
                                    self._ptr(keys), self._ptr(counts), _u64(base), _u64(nslots), self._ptr(table_status),
                                    _u32(lo), _u32(hi), self._ptr(out), _u64(out_offs), int(out.numel()), self._ptr(d_lens),
                                    self._ptr(d_rows), self._ptr(d_status), self._ptr(ws), ws.numel())
        _capi.check(self.ctx, st, "vk_depth_device")
        # (the copies below wait for the kernels: the workspace is free after them)
        return (d_lens[:n].cpu().numpy().astype(np.uint64), d_rows[:n].cpu().numpy().view(np.uint64),
                d_status[:n].cpu().numpy().astype(np.uint32))

    @staticmethod
    def _sketch_args(s, m):
        s, m = int(s), int(m)
        if not _capi.VK_SKETCH_MIN <= s <= _capi.VK_SKETCH_MAX:
            raise ValueError(f"a sketch holds {_capi.VK_SKETCH_MIN}..{_capi.VK_SKETCH_MAX} hashes: {s}")
        if not 1 <= m < 2 ** 32:
            raise ValueError(f"the sketch's minimum multiplicity is at least 1: {m}")
        return s, m

    def sketch_tables(self, keys, counts, base, nslots, status, s, m=1):
        """The bottom-s MinHash sketches of counting tables in HBM (vk_sketch_device): sample i owns slots base[i] .. +
        nslots[i] of keys (int64 device tensor, a free slot all ones) and counts (int32 device tensor), status an int32
        device tensor [n] (a sample with a status gets an empty sketch); a held slot is eligible when its count is at
        least m.  Returns (hashes uint64[n, s]: the min(s, eligible) smallest mixes of eligible keys, ascending, then all
        ones; info uint64[n, 2]: eligible, length).  Synchronises."""
        torch = _torch()
        s, m = self._sketch_args(s, m)
        base = np.ascontiguousarray(base, dtype=np.uint64)
        nslots = np.ascontiguousarray(nslots, dtype=np.uint64)
        n = len(nslots)
        if len(base) != n or int(status.numel()) != n:
            raise ValueError("one base, one slot count and one status per sample")
        if n and int((base + nslots).max()) > min(int(keys.numel()), int(counts.numel())):
            raise ValueError("a sample's slots lie past the tables")
        ws = self._workspace(self.L.vk_sketch_workspace_size, _u64(nslots), n, s)
        d_hashes = torch.empty((n, s), dtype=torch.int64, device=self.device)
        d_info = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        st = self.L.vk_sketch_device(self.ctx, self._ptr(keys), self._ptr(counts), _u64(base), _u64(nslots), n, self._ptr(status),
                                     m, s, self._ptr(d_hashes), self._ptr(d_info), self._ptr(ws), ws.numel())
        _capi.check(self.ctx, st, "vk_sketch_device")
        # (the copies below wait for the kernels: the workspace is free after them)
        return d_hashes.cpu().numpy().view(np.uint64), d_info.cpu().numpy().view(np.uint64)

    def sketch_pairs(self, q, qlen, r, rlen, s):
        """Every query sketch against every reference sketch (vk_sketch_pairs_device): q uint64[nq, s] with lengths
        qlen[nq], r and rlen likewise (NumPy arrays, rows ascending in their first length entries; `r is q` compares a set
        with itself).  Returns (shared uint32[nq, nr], seen uint32[nq, nr]): seen = min(s, |Sa u Sb|), shared = the values
        among the seen smallest of the union that lie in both.  Synchronises."""
        torch = _torch()
        s = self._sketch_args(s, 1)[0]

        def up(h, ln):
            h = np.ascontiguousarray(h, dtype=np.uint64)
            ln = np.ascontiguousarray(ln, dtype=np.uint64)
            if h.ndim != 2 or h.shape[1] != s or ln.shape != (h.shape[0],):
                raise ValueError(f"sketches are uint64 [n, {s}] with one length each")
            if len(ln) and int(ln.max()) > s:
                raise ValueError("a sketch is longer than its row")
            return (torch.from_numpy(h.view(np.int64)).to(self.device), torch.from_numpy(ln.view(np.int64)).to(self.device))
        dq, dql = up(q, qlen)
        dr, drl = (dq, dql) if r is q else up(r, rlen)
        nq, nr = int(dq.shape[0]), int(dr.shape[0])
        if nq == 0 or nr == 0:
            return np.zeros((nq, nr), dtype=np.uint32), np.zeros((nq, nr), dtype=np.uint32)
        shared = torch.empty((nq, nr), dtype=torch.int32, device=self.device)
        seen = torch.empty((nq, nr), dtype=torch.int32, device=self.device)
        st = self.L.vk_sketch_pairs_device(self.ctx, self._ptr(dq), self._ptr(dql), nq, self._ptr(dr), self._ptr(drl), nr, s,
                                           self._ptr(shared), self._ptr(seen))
        _capi.check(self.ctx, st, "vk_sketch_pairs_device")
        return shared.cpu().numpy().view(np.uint32), seen.cpu().numpy().view(np.uint32)

    def sketch_pair_blocks(self, q, qlen, r, rlen, s):
        """sketch_pairs with both counts split by block (vk_sketch_pair_blocks_device; `tree --replicates`): a value h
        belongs to block h & 63.  Returns (shared uint32[nq, nr, 64], seen uint32[nq, nr, 64]); over the last axis they
        sum to sketch_pairs' two outputs.  nq * nr is at most 2^26.  Synchronises."""
        torch = _torch()
        s = self._sketch_args(s, 1)[0]

        def up(h, ln):
            h = np.ascontiguousarray(h, dtype=np.uint64)
            ln = np.ascontiguousarray(ln, dtype=np.uint64)
            if h.ndim != 2 or h.shape[1] != s or ln.shape != (h.shape[0],):
                raise ValueError(f"sketches are uint64 [n, {s}] with one length each")
            if len(ln) and int(ln.max()) > s:
                raise ValueError("a sketch is longer than its row")
            return (torch.from_numpy(h.view(np.int64)).to(self.device), torch.from_numpy(ln.view(np.int64)).to(self.device))
        dq, dql = up(q, qlen)
        dr, drl = (dq, dql) if r is q else up(r, rlen)
        nq, nr, nb = int(dq.shape[0]), int(dr.shape[0]), _capi.VK_SKETCH_BLOCKS
        if nq == 0 or nr == 0:
            return np.zeros((nq, nr, nb), dtype=np.uint32), np.zeros((nq, nr, nb), dtype=np.uint32)
        if nq * nr > 1 << 26:
            raise ValueError(f"per-block counts of at most 2^26 pairs in a call: {nq} x {nr}")
        shared = torch.empty((nq, nr, nb), dtype=torch.int32, device=self.device)
        seen = torch.empty((nq, nr, nb), dtype=torch.int32, device=self.device)
        st = self.L.vk_sketch_pair_blocks_device(self.ctx, self._ptr(dq), self._ptr(dql), nq, self._ptr(dr), self._ptr(drl), nr, s,
                                                 self._ptr(shared), self._ptr(seen))
        _capi.check(self.ctx, st, "vk_sketch_pair_blocks_device")
        return shared.cpu().numpy().view(np.uint32), seen.cpu().numpy().view(np.uint32)

    def nj(self, dist):
        """Neighbour-joining trees of a batch of distance matrices (vk_tree_nj_device; the rule: INTEGRATION.md, "`tree`:
        the rule"): dist float64 [ntrees, n, n] or [n, n] (a NumPy array, left as it is).  Returns (status uint32[ntrees]:
        0 or VK_TREE_BAD_VALUE, nodes uint32[ntrees, 2 (n - 3) + 3], lengths float64 of the same shape): step t joined
        slots nodes[2t] < nodes[2t + 1] with those branch lengths, the last three entries are the closing slots; a matrix
        with a status has an all-zero record.  Synchronises."""
        torch = _torch()
        d = np.ascontiguousarray(dist, dtype=np.float64)
        if d.ndim == 2:
            d = d[None]
        if d.ndim != 3 or d.shape[1] != d.shape[2]:
            raise ValueError("distance matrices are float64 [ntrees, n, n]")
        ntrees, n = int(d.shape[0]), int(d.shape[1])
        if not _capi.VK_TREE_MIN_LEAVES <= n <= _capi.VK_TREE_MAX_LEAVES or not 1 <= ntrees <= _capi.VK_TREE_MAX_TREES:
            raise ValueError(f"a tree has {_capi.VK_TREE_MIN_LEAVES}..{_capi.VK_TREE_MAX_LEAVES} leaves and a call 1.."
                             f"{_capi.VK_TREE_MAX_TREES} trees: {n} leaves, {ntrees} trees")
        if not d.flags.writeable:
            d = d.copy()
        dd = torch.from_numpy(d).to(self.device)   # (the device's copy is overwritten)
        return self.nj_device(dd)

    def nj_device(self, dd):
        """nj on a float64 device tensor [ntrees, n, n], which is OVERWRITTEN."""
        torch = _torch()
        ntrees, n = int(dd.shape[0]), int(dd.shape[1])
        rec = 2 * (n - 3) + 3
        ws = self._workspace(self.L.vk_tree_workspace_size, n, ntrees)
        nodes = torch.empty((ntrees, rec), dtype=torch.int32, device=self.device)
        lengths = torch.empty((ntrees, rec), dtype=torch.float64, device=self.device)
        status = torch.empty((ntrees,), dtype=torch.int32, device=self.device)
        st = self.L.vk_tree_nj_device(self.ctx, self._ptr(dd), n, ntrees, self._ptr(nodes), self._ptr(lengths), self._ptr(status),
                                      self._ptr(ws), ws.numel())
        _capi.check(self.ctx, st, "vk_tree_nj_device")
        # (the copies below wait for the kernels: the workspace is free after them)
        return status.cpu().numpy().view(np.uint32), nodes.cpu().numpy().view(np.uint32), lengths.cpu().numpy()

    def neighbours(self, q, r, n=10, qgroup=None, rgroup=None, matrix=False):
        """The n nearest references of every query image by exact squared Euclidean distance (vk_dist_device; the rule:
        INTEGRATION.md, "`compare`: the rule").  q, r: uint8 device tensors [nq, side, side] or [nq, P] of equal P; `q is
        r` compares a set with itself.  qgroup, rgroup: group ids (uint32 values, 0xFFFFFFFF = no group), both or
        neither: a reference of a query's own group is no neighbour of it.  Returns (idx uint32[nq, n], d2 uint64[nq, n])
        as NumPy arrays, slots without a reference 0xFFFFFFFF and 2^64 - 1; with matrix=True also every distance as an
        int64 device tensor [nq, nr] (the values are below 2^63).  Synchronises."""
        torch = _torch()

        def rows(t):
            if t.dtype != torch.uint8 or t.device != self.device or t.dim() not in (2, 3):
                raise ValueError("images are uint8 tensors [n, side, side] or [n, P] on the engine's device")
            return t.reshape(t.shape[0], -1).contiguous()
        q2 = rows(q)
        r2 = q2 if r is q else rows(r)
        nq, npix = (int(v) for v in q2.shape)
        nr = int(r2.shape[0])
        if int(r2.shape[1]) != npix:
            raise ValueError("queries and references differ in size")
        if (qgroup is None) != (rgroup is None):
            raise ValueError("group ids for both sides or for neither")
        n = int(n)
        groups = [None, None]
        if qgroup is not None:
            for i, (g, count) in enumerate(((qgroup, nq), (rgroup, nr))):
                g = np.array(g, dtype=np.uint32)   # (a copy: the caller's may be read-only)
                if g.shape != (count,):
                    raise ValueError("one group id per image")
                groups[i] = torch.from_numpy(g.view(np.int32)).to(self.device)
        ws = self._workspace(self.L.vk_dist_workspace_size, nq, nr, npix, n if 0 <= n < 2 ** 32 else 0, int(matrix))
        idx = torch.empty((nq, n), dtype=torch.int32, device=self.device)
        d2 = torch.empty((nq, n), dtype=torch.int64, device=self.device)
        mat = torch.empty((nq, nr), dtype=torch.int64, device=self.device) if matrix else None
        st = self.L.vk_dist_device(self.ctx, self._ptr(q2), nq, self._ptr(r2), nr, npix,
                                   self._ptr(groups[0]) if qgroup is not None else None,
                                   self._ptr(groups[1]) if qgroup is not None else None, n, self._ptr(idx), self._ptr(d2),
                                   self._ptr(mat) if matrix else None, self._ptr(ws), ws.numel())
        _capi.check(self.ctx, st, "vk_dist_device")
        # (the copies below wait for the kernels: the workspace is free after them)
        out = (idx.cpu().numpy().view(np.uint32), d2.cpu().numpy().view(np.uint64))
        return out + (mat,) if matrix else out

    def deflate_bound(self, lengths):
        """Bytes that the files of texts of these lengths take at most (vk_deflate_bound)."""
        lens = np.ascontiguousarray(lengths, dtype=np.uint64)
        b = C.c_uint64()
        _capi.check(self.ctx, self.L.vk_deflate_bound(_u64(lens), len(lens), C.byref(b)), "vk_deflate_bound")
        return int(b.value)

    def deflate(self, text, offs, lens):
        """The texts text[offs[i] .. +lens[i]) (a uint8 device tensor; offsets multiples of 16) as one BGZF .fq.gz file
        each, compressed where they lie (vk_deflate_device).  Returns (uint8 device tensor, file offsets uint64[n], file
        lengths uint64[n]): the files lie packed in the order given, so [0, offsets[-1] + lengths[-1]) is all there is
        to copy back.  Synchronises."""
        torch = _torch()
        offs, lens = self._desc(offs, lens)
        n = len(offs)
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device=self.device), offs, lens
        ws = self._workspace(self.L.vk_deflate_workspace_size, _u64(lens), n)
        cap = self.deflate_bound(lens)
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        out_offs = np.zeros(n, dtype=np.uint64)
        out_lens = np.zeros(n, dtype=np.uint64)
        _capi.check(self.ctx, self.L.vk_deflate_device(self.ctx, self._ptr(text), _u64(offs), _u64(lens), n, self._ptr(out), cap,
                                                       self._ptr(ws), ws.numel(), _u64(out_offs), _u64(out_lens)),
                    "vk_deflate_device")
        return out, out_offs, out_lens

    def png(self, img):
        """The IDAT chunks of the images img [n, side, side] (a uint8 device tensor), encoded where they lie
        (vk_png_device): a list of n bytes objects, each a complete chunk (length, "IDAT", zlib stream, CRC-32) that
        image.write_png_parts puts between a file's head and IEND.  The images are taken in calls whose output and
        workspace stay within PNG_CALL_BYTES; each call is one copy back of the bytes it wrote.  Synchronises."""
        torch = _torch()
        n, side = int(img.shape[0]), int(img.shape[1])
        if n == 0:
            return []
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == side and img.is_contiguous()
        bound, ws_bytes = C.c_uint64(), C.c_uint64()
        _capi.check(self.ctx, self.L.vk_png_bound(side, 1, C.byref(bound)), "vk_png_bound")
        _capi.check(self.ctx, self.L.vk_png_workspace_size(side, 1, C.byref(ws_bytes)), "vk_png_workspace_size")
        per_call = max(1, min(n, PNG_CALL_BYTES // int(bound.value + ws_bytes.value)))
        _capi.check(self.ctx, self.L.vk_png_bound(side, per_call, C.byref(bound)), "vk_png_bound")
        _capi.check(self.ctx, self.L.vk_png_workspace_size(side, per_call, C.byref(ws_bytes)), "vk_png_workspace_size")
        out = torch.empty(int(bound.value), dtype=torch.uint8, device=self.device)
        ws = torch.empty(max(int(ws_bytes.value), 256), dtype=torch.uint8, device=self.device)
        offs, lens = np.zeros(per_call, dtype=np.uint64), np.zeros(per_call, dtype=np.uint64)
        chunks = []
        for i0 in range(0, n, per_call):
            m = min(per_call, n - i0)
            _capi.check(self.ctx, self.L.vk_png_device(self.ctx, self._ptr(img[i0:i0 + m]), m, side, self._ptr(out), out.numel(),
                                                       self._ptr(ws), ws.numel(), _u64(offs), _u64(lens)), "vk_png_device")
            host = out[:int(offs[m - 1] + lens[m - 1])].cpu().numpy()
            chunks.extend(host[int(o):int(o + ln)].tobytes() for o, ln in zip(offs[:m], lens[:m]))
        return chunks

    def unpng(self, streams, side):
        """The images of n PNG files' zlib streams, decoded on the GPU (vk_unpng_device): a uint8 device tensor
        [n, side, side] and the status array [n] (0, or VK_UNPNG_* bits: that image's pixels mean nothing).
        streams = (buffer, offsets, lengths): a host uint8 tensor or array laid out as pngread.pack_streams does (every
        stream at a multiple of 16, the four length bytes behind it, pngread.SLACK bytes behind the last).  The streams
        are taken in calls whose bytes, images and workspace stay within PNG_CALL_BYTES.  Synchronises."""
        torch = _torch()
        buf, offs, lens = streams
        buf = buf if torch.is_tensor(buf) else torch.from_numpy(buf)
        offs, lens = np.ascontiguousarray(offs, dtype=np.uint64), np.ascontiguousarray(lens, dtype=np.uint64)
        n = len(offs)
        img = torch.empty((n, side, side), dtype=torch.uint8, device=self.device)
        status = np.zeros(n, dtype=np.uint32)
        if n == 0:
            return img, status
        ws1 = C.c_uint64()
        _capi.check(self.ctx, self.L.vk_unpng_workspace_size(side, 1, C.byref(ws1)), "vk_unpng_workspace_size")
        ends = np.append(offs[1:], np.uint64((int(offs[-1] + lens[-1]) + 15) // 16 * 16)).astype(np.int64)
        i0 = 0
        while i0 < n:
            # as many images as fit the budget (at least one): their streams, and per image a workspace share
            base = int(offs[i0])
            cost = (ends[i0:] - base) + (np.arange(1, n - i0 + 1, dtype=np.int64) * int(ws1.value + 64))
            m = max(1, int(np.searchsorted(cost, PNG_CALL_BYTES, side="right")))
            ws = self._workspace(self.L.vk_unpng_workspace_size, side, m)
            end = int(ends[i0 + m - 1])
            dev = torch.zeros(end - base + 1024, dtype=torch.uint8, device=self.device)
            dev[:end - base].copy_(buf[base:end])
            rel = offs[i0:i0 + m] - np.uint64(base)
            st = status[i0:i0 + m].ctypes.data_as(C.POINTER(C.c_uint32))
            _capi.check(self.ctx, self.L.vk_unpng_device(self.ctx, self._ptr(dev), _u64(rel), _u64(lens[i0:i0 + m]), m, side,
                                                         self._ptr(img[i0:i0 + m]), st, self._ptr(ws), ws.numel()),
                        "vk_unpng_device")
            i0 += m
        return img, status

    def images(self, hist, img=None):
        """K2: uint8 images [n, side, side] from histograms [n, 4^k]."""
        torch = _torch()
        n = hist.shape[0]
        if img is None:
            img = torch.empty((n, self.side, self.side), dtype=torch.uint8, device=self.device)
        st = self.L.vk_image_device(self.ctx, self._ptr(hist), n, self.k, self._ptr(img))
        _capi.check(self.ctx, st, "vk_image_device")
        return img

    def fastq_to_images(self, fastq, offsets, lengths, parts=0, hist=None, status=None, img=None):
        torch = _torch()
        offs, lens = self._desc(offsets, lengths)
        n = len(offs)
        if hist is None:
            hist = torch.empty((n, self.ncode), dtype=torch.int32, device=self.device)
        if status is None:
            status = torch.empty((n,), dtype=torch.int32, device=self.device)
        if img is None:
            img = torch.empty((n, self.side, self.side), dtype=torch.uint8, device=self.device)
        st = self.L.vk_fastq_to_image_device(self.ctx, self._ptr(fastq), _u64(offs), _u64(lens), n, self.k, parts,
                                             self._ptr(hist), self._ptr(status), self._ptr(img))
        _capi.check(self.ctx, st, "vk_fastq_to_image_device")
        return img, hist, status

    def synth(self, sample0, nsamples, reads, readlen=150, seed=20250824, dist=0, out=None):
        """Synthetic FASTQ for samples sample0..sample0+nsamples-1, generated in HBM (dist 0, 1: records of one
        size; dist 2: reads shaped like fastp's output, samples of different sizes -- synth.py)."""
        torch = _torch()
        if dist == 2:
            lens = np.zeros(nsamples, dtype=np.uint64)
            _capi.check(self.ctx, self.L.vk_synth_shaped_lengths(self.ctx, sample0, nsamples, reads, readlen, C.c_uint64(seed),
                                                                  _u64(lens)), "vk_synth_shaped_lengths")
            offs = np.zeros(nsamples, dtype=np.uint64)
            if nsamples > 1:
                offs[1:] = np.cumsum((lens[:-1] + np.uint64(15)) // np.uint64(16) * np.uint64(16))
            total = int(offs[-1] + lens[-1]) if nsamples else 0
            if out is None or out.numel() < (total + 15) // 16 * 16 + 16:
                out = torch.empty(((total + 15) // 16 * 16 + 16,), dtype=torch.uint8, device=self.device)
            _capi.check(self.ctx, self.L.vk_synth_shaped_device(self.ctx, self._ptr(out), _u64(offs), sample0,
                                                                 nsamples, reads, readlen, C.c_uint64(seed)), "vk_synth_shaped_device")
            return out, offs, lens
        rec = 2 * readlen + 20
        total = rec * reads * nsamples
        if out is None:
            out = torch.empty(((total + 15) // 16 * 16 + 16,), dtype=torch.uint8, device=self.device)
        st = self.L.vk_synth_fastq_device(self.ctx, self._ptr(out), sample0, nsamples, reads, readlen,
                                          C.c_uint64(seed), dist)
        _capi.check(self.ctx, st, "vk_synth_fastq_device")
        offs = np.arange(nsamples, dtype=np.uint64) * np.uint64(rec * reads)
        lens = np.full(nsamples, rec * reads, dtype=np.uint64)
        return out, offs, lens

    def last_count_launch(self):
        g, b, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.L.vk_last_count_launch(self.ctx, C.byref(g), C.byref(b), C.byref(l))
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value}

    def last_count_pull(self, nsamples):
        """(helpers allowed per sample, flushes per sample) of the last k <= 7 count; every flush count 0: it was no pulling launch"""
        h, f = C.c_uint32(), (C.c_uint32 * max(nsamples, 1))()
        _capi.check(self.ctx, self.L.vk_last_count_pull(self.ctx, C.byref(h), f, nsamples), "vk_last_count_pull")
        return h.value, list(f)[:nsamples]

    def last_count_general(self):
        """(pieces of the last k <= 7 count that took the general path, pieces in all)"""
        g, n = C.c_uint64(), C.c_uint64()
        _capi.check(self.ctx, self.L.vk_last_count_general(self.ctx, C.byref(g), C.byref(n)), "vk_last_count_general")
        return g.value, n.value

    # -- host conveniences -------------------------------------------------------
    def count_host(self, data):
        """One host FASTQ byte string -> (hist uint32[4^k], status bits)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
        hist = np.empty(self.ncode, dtype=np.uint32)
        stw = C.c_uint32(0)
        st = self.L.vk_count_host(self.ctx, C.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, self.k, _u32(hist),
                                  C.byref(stw))
        if st not in (_capi.VK_OK, _capi.VK_EFORMAT):
            _capi.check(self.ctx, st, "vk_count_host")
        return hist, stw.value

    def count_fasta_host(self, data):
        """One host FASTA byte string -> (hist uint32[4^k], status bits, sequence bytes)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
        hist = np.empty(self.ncode, dtype=np.uint32)
        stw = C.c_uint32(0)
        nb = C.c_uint64(0)
        st = self.L.vk_count_fasta_host(self.ctx, C.c_void_p(buf.ctypes.data if buf.size else 0), buf.size, self.k, _u32(hist),
                                        C.byref(stw), C.byref(nb))
        if st not in (_capi.VK_OK, _capi.VK_EFORMAT):
            _capi.check(self.ctx, st, "vk_count_fasta_host")
        return hist, stw.value, nb.value

    def image_host(self, hist):
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        img = np.empty(self.npix, dtype=np.uint8)
        st = self.L.vk_image_host(self.ctx, _u32(hist), self.k, _u8(img))
        _capi.check(self.ctx, st, "vk_image_host")
        return img.reshape(self.side, self.side)


def count_giant_sample(engine, data, rank=0, world=1):
    """ONE sample spread over the ranks of a torch.distributed job (optional row): every
    rank counts a record-aligned byte range of the FASTQ text on its own GPU, then the 4^k u32
    histograms are summed with one all-reduce (RCCL when the group is nccl).  Returns the full
    histogram tensor (identical on every rank) and this rank's status word."""
    from .shard import allreduce_sum_, split_at_records, widen_u32
    start, end = split_at_records(data, world)[rank]
    part = data[start:end]
    dev, offs, lens = engine.upload([part])
    hist, status = engine.count(dev, offs, lens)
    h = widen_u32(hist.view(-1))              # sum in 64 bit (unsigned widening): counts of a giant sample may pass 2^31
    allreduce_sum_(h)
    return h, int(status.cpu()[0])
