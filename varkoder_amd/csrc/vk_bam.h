// vk_bam.h -- BAM records in HBM -> FASTQ text in HBM: `image / query --from-bam` (vk_bam_frame_device,
// vk_bam_fastq_device).  Part of the one translation unit vkimg.hip.
//
// The rule ("--from-bam: the rule"; tests/bam_ref.py is the same rule in Python; SAM spec section 4.2): a
// file's inflated bytes hold a header and then records, each a block_size word and block_size bytes.  A record with
// l_seq > 0 and no flag bit of `exclude` becomes a read of l_read_name + 2 * l_seq + 5 bytes of text; a stream takes
// every read of its file (VK_BAM_ALL) or those of one class (READ1, READ2, SINGLE).
//
// Framing: speculate, then verify.  A record's start is known only from the record before it, so the chain of block_size
// words is serial.  What the calls return never depends on a guess; only their speed does.
//     vk_bam_segment_kernel   a wavefront per segment of kBamSegBytes (VKIMG_BAM_SEG_BYTES): segment 0 enters at
//                             first_record, any other guesses its entry -- the smallest offset among its bytes at which a
//                             plausible record starts and kBamChain plausible records follow -- and walks from there to the
//                             first record at or past its end, tallying records and text bytes per class and noting
//                             where every record starts (a u16 behind the segment's start)
//     vk_bam_link_kernel      a wavefront per file carries the TRUE entry through the segments, 64 at a step: a run of
//                             segments each of whose guesses equals the exit of the one before it stands as it is; the
//                             first that does not is walked again from the true entry (rewalked), or starts no record
//                             (true entry at or past its end: a record longer than a segment).  The same pass sums the
//                             tallies: every segment learns where its text begins in the text of every class
//     vk_bam_emit_kernel      a workgroup per (stream, segment) takes the segment's records 64 at a time from the noted
//                             starts (no hop from record to record here); a wave prefix sum over their text sizes places
//                             them, and the lanes of the workgroup are spread over aligned 16-byte blocks of OUTPUT text, not
//                             over records
// Records and their fields are not aligned (a name of even length misaligns all that follows): every field is put
// together from byte loads.  Nothing is read past a file's length, nothing is written outside a stream's slot.
//
// The lane-local code -- field reads, the validity check, the predicate of a guess, a record's class and size, the walk of
// a segment, the text of a byte range of a record -- compiles for the host under VK_BAM_LANE_ONLY:
// tests/emul/bam_emul.cpp.
#ifndef VK_BAM_H
#define VK_BAM_H

namespace {

constexpr uint32_t kBamBadRecord = 1, kBamTruncated = 2;                         // VK_BAM_BAD_RECORD, VK_BAM_TRUNCATED
constexpr uint32_t kBamAll = 0, kBamRead1 = 1, kBamRead2 = 2, kBamSingle = 3;    // VK_BAM_ALL .. VK_BAM_SINGLE
constexpr uint32_t kBamNoGuess = 1;                                              // VK_BAM_NO_GUESS
constexpr uint32_t kBamSegBytes = 65536;   // bytes of a segment (VKIMG_BAM_SEG_BYTES: 64 .. 65536, a record's start behind its segment's is a u16)
constexpr uint32_t kBamMinRecord = 37;     // block_size word, 32 bytes of fields, a name of one NUL: what bam_read lets pass
constexpr uint32_t kBamChain = 3;          // plausible records that must follow a guessed one
constexpr uint64_t kBamNone = ~0ull;       // a segment without a guess

__device__ inline uint32_t bam_u16(const uint8_t* p) { return p[0] | static_cast<uint32_t>(p[1]) << 8; }
__device__ inline uint32_t bam_u32(const uint8_t* p) {
    return p[0] | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
}

// The fields of a record that the conversion reads (offsets within the block, SAM spec 4.2: refID 0, l_read_name 8,
// n_cigar_op 12, flag 14, l_seq 16, next_refID 20, read_name 32).
struct BamRec {
    uint64_t at;   // of its block_size word, within the file
    uint32_t block_size, l_name, n_cigar, flag, l_seq;
    int32_t ref_id, next_ref_id;
};

// The record at `at` (p, len: the file): 0, or the status it gives the file.  A record that runs past the file's end is
// VK_BAM_TRUNCATED; a block_size too small for the fixed fields, or for the name, cigar, bases and qualities these state,
// an empty name and a name that does not end in NUL are VK_BAM_BAD_RECORD.
__device__ inline uint32_t bam_read(const uint8_t* p, uint64_t len, uint64_t at, BamRec* r) {
    if (at > len || len - at < 4) return kBamTruncated;
    const uint32_t bs = bam_u32(p + at);
    if (bs >= 0x80000000u || bs < 32) return kBamBadRecord;
    if (len - at - 4 < bs) return kBamTruncated;
    const uint8_t* f = p + at + 4;
    r->at = at;
    r->block_size = bs;
    r->ref_id = static_cast<int32_t>(bam_u32(f));
    r->l_name = f[8];
    r->n_cigar = bam_u16(f + 12);
    r->flag = bam_u16(f + 14);
    r->l_seq = bam_u32(f + 16);
    r->next_ref_id = static_cast<int32_t>(bam_u32(f + 20));
    const uint64_t need = 32ull + r->l_name + 4ull * r->n_cigar + (static_cast<uint64_t>(r->l_seq) + 1) / 2 + r->l_seq;
    if (r->l_name == 0 || bs < need) return kBamBadRecord;
    if (f[32 + r->l_name - 1] != 0) return kBamBadRecord;
    return 0;
}

// What a guess asks of a record on top of bam_read: reference ids the header knows, a printable name.
__device__ inline bool bam_plausible(const uint8_t* p, uint64_t len, int32_t n_ref, uint64_t at, BamRec* r) {
    if (bam_read(p, len, at, r)) return false;
    if (r->ref_id < -1 || r->ref_id >= n_ref || r->next_ref_id < -1 || r->next_ref_id >= n_ref) return false;
    const uint8_t* name = p + at + 36;
    for (uint32_t j = 0; j + 1 < r->l_name; ++j)
        if (name[j] < '!' || name[j] > '~') return false;
    return true;
}

// Candidate c as a segment's entry: a plausible record, and kBamChain more behind it (or the file's end).
__device__ inline bool bam_guess_ok(const uint8_t* p, uint64_t len, int32_t n_ref, uint64_t c) {
    BamRec r;
    uint64_t at = c;
#pragma unroll 1   // (unrolled, the nested tests of four records spill scalar registers in the segment kernel)
    for (uint32_t i = 0; i <= kBamChain; ++i) {
        if (i && at == len) return true;
        if (!bam_plausible(p, len, n_ref, at, &r)) return false;
        at += 4ull + r.block_size;
    }
    return true;
}

// 0: not a read (no bases, or a flag bit of `exclude`); else the class of the read.
__device__ inline uint32_t bam_class(const BamRec& r, uint32_t exclude) {
    if (r.l_seq == 0 || (r.flag & exclude)) return 0;
    const uint32_t m = r.flag & 0xC1u;
    return m == 0x41u ? kBamRead1 : m == 0x81u ? kBamRead2 : kBamSingle;
}
__device__ inline bool bam_takes(uint32_t select, uint32_t cls) { return cls && (select == kBamAll || select == cls); }
__device__ inline uint64_t bam_text_size(const BamRec& r) { return r.l_name + 2ull * r.l_seq + 5; }

struct BamTally {
    uint64_t recs[3], bytes[3];   // per class: READ1, READ2, SINGLE
};

// The starts a segment of seg_bytes can hold: one per kBamMinRecord bytes.
// (the host sizes its workspaces with it: vk_bamplan.h.  A lane-only build has no `__host__`: its `__device__` is empty)
#ifdef VK_BAM_LANE_ONLY
#define VK_BAM_HOST
#else
#define VK_BAM_HOST __host__
#endif
VK_BAM_HOST __device__ inline uint32_t bam_starts_cap(uint32_t seg_bytes) { return seg_bytes / kBamMinRecord + 2; }

// From the record at `at` to the first that starts at or past `end`: the reads of each class and their text bytes.
// Returns 0 or the status of the record it stopped at; *exit = that record, or the first one past the end.
// starts[0 .. *nrec): where each valid record of the walk starts, behind seg_start (at >= seg_start, end - seg_start <=
// 65536; at most cap are noted, and a walk from a true entry has no more).
__device__ inline uint32_t bam_walk(const uint8_t* p, uint64_t len, uint64_t at, uint64_t end, uint32_t exclude, BamTally* t,
                                    uint64_t* exit, uint64_t seg_start, uint16_t* starts, uint32_t cap, uint32_t* nrec) {
    for (uint32_t c = 0; c < 3; ++c) t->recs[c] = t->bytes[c] = 0;
    uint32_t st = 0, n = 0;
    while (at < end) {
        BamRec r;
        st = bam_read(p, len, at, &r);
        if (st) break;
        if (n < cap) starts[n++] = static_cast<uint16_t>(at - seg_start);
        const uint32_t cls = bam_class(r, exclude);
        if (cls) {
            t->recs[cls - 1] += 1;
            t->bytes[cls - 1] += bam_text_size(r);
        }
        at += 4ull + r.block_size;
    }
    *exit = at;
    *nrec = n;
    return st;
}

// What the text of a read is made from.
struct BamEmit {
    const uint8_t* rec;          // the block (behind the block_size word)
    uint64_t seq_off, qual_off;  // within the block
    uint32_t l_name, l_seq;
    uint32_t reverse, no_qual;   // flag & 0x10; the first quality byte is 0xFF
};

__device__ inline BamEmit bam_emit_of(const uint8_t* p, const BamRec& r) {
    BamEmit e;
    e.rec = p + r.at + 4;
    e.l_name = r.l_name;
    e.l_seq = r.l_seq;
    e.seq_off = 32ull + r.l_name + 4ull * r.n_cigar;
    e.qual_off = e.seq_off + (static_cast<uint64_t>(r.l_seq) + 1) / 2;
    e.reverse = (r.flag & 0x10u) ? 1u : 0u;
    e.no_qual = r.l_seq && e.rec[e.qual_off] == 0xFF ? 1u : 0u;
    return e;
}

// The letter of a 4-bit base code ("=ACMGRSVTWYHKDBN", '=' written as N).  The code is a set of bases, A = 1, C = 2,
// G = 4, T = 8: its complement is the code with the four bits in reverse order.
__device__ inline uint8_t bam_base(uint32_t code, uint32_t reverse) {
    if (reverse) code = ((code & 1u) << 3) | ((code & 2u) << 1) | ((code & 4u) >> 1) | ((code & 8u) >> 3);
    const uint64_t lo = 0x565352474D43414Eull;                    // N A C M G R S V (byte 0 first)
    const uint64_t hi = 0x4E42444B48595754ull;                    // T W Y H K D B N
    return static_cast<uint8_t>(((code & 8u) ? hi : lo) >> (8 * (code & 7u)));
}

// The per-byte routine and what wraps it are inlined into every kernel that writes text (two do: vk_bam_emit_kernel here,
// vk_bam_groups_emit_kernel in vk_bam_groups.h): left to the compiler, a second caller turns bam_emit_item into a call and
// the emit pass loses a fifth of its speed.
#define VK_BAM_INLINE __attribute__((always_inline))

// Byte i of a read's text: '@' name '\n' SEQ '\n' '+' '\n' QUAL '\n'.
__device__ inline VK_BAM_INLINE uint8_t bam_text_byte(const BamEmit& e, uint64_t i) {
    if (i == 0) return '@';
    if (i < e.l_name) return e.rec[32 + i - 1];
    if (i == e.l_name) return '\n';
    uint64_t q = i - e.l_name - 1;
    if (q < e.l_seq) {
        const uint64_t at = e.reverse ? e.l_seq - 1 - q : q;
        const uint32_t b = e.rec[e.seq_off + (at >> 1)];
        return bam_base((at & 1) ? b & 15u : b >> 4, e.reverse);
    }
    q -= e.l_seq;
    if (q < 3) return q == 1 ? '+' : '\n';
    q -= 3;
    if (q < e.l_seq) {
        if (e.no_qual) return 'I';
        const uint32_t v = e.rec[e.qual_off + (e.reverse ? e.l_seq - 1 - q : q)];
        return static_cast<uint8_t>((v > 93 ? 93u : v) + 33u);
    }
    return '\n';
}

constexpr uint32_t kBamItemBytes = 16;   // an item of the emit pass: one aligned 16-byte block of output text

struct alignas(16) BamQuad {
    uint32_t w[4];
};

__device__ inline VK_BAM_INLINE uint32_t bam_text_word(const BamEmit& e, uint64_t i) {
    return bam_text_byte(e, i) | static_cast<uint32_t>(bam_text_byte(e, i + 1)) << 8 |
           static_cast<uint32_t>(bam_text_byte(e, i + 2)) << 16 | static_cast<uint32_t>(bam_text_byte(e, i + 3)) << 24;
}

// Bytes [lo, hi) of a read's text to out (the place of byte lo), each store as wide as the output's alignment allows:
// bytes up to a dword boundary, dwords up to a 16-byte boundary, 16-byte stores, dwords, bytes.
__device__ inline VK_BAM_INLINE void bam_emit_range(const BamEmit& e, uint64_t lo, uint64_t hi, uint8_t* out) {
    uint64_t i = lo;
    for (; i < hi && (reinterpret_cast<uintptr_t>(out) & 3u); ++i) *out++ = bam_text_byte(e, i);
    while (hi - i >= 4) {
        if (hi - i >= 16 && !(reinterpret_cast<uintptr_t>(out) & 15u)) {
            BamQuad q;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) q.w[k] = bam_text_word(e, i + 4 * k);
            *reinterpret_cast<BamQuad*>(out) = q;
            i += 16;
            out += 16;
        } else {
            *reinterpret_cast<uint32_t*>(out) = bam_text_word(e, i);
            i += 4;
            out += 4;
        }
    }
    for (; i < hi; ++i) *out++ = bam_text_byte(e, i);
}

// A read's text of `size` bytes at `out` is written in items: one per aligned block of kBamItemBytes of the output it
// touches (whole blocks by one store, a read's two ends by narrower ones: neighbours in the text write the rest).
__device__ inline uint64_t bam_items(const uint8_t* out, uint64_t size) {
    const uint64_t a = reinterpret_cast<uintptr_t>(out) & (kBamItemBytes - 1);
    return size ? (a + size + kBamItemBytes - 1) / kBamItemBytes : 0;
}
__device__ inline VK_BAM_INLINE void bam_emit_item(const BamEmit& e, uint8_t* out, uint64_t size, uint64_t item) {
    const uint64_t a = reinterpret_cast<uintptr_t>(out) & (kBamItemBytes - 1);
    const uint64_t lo = item ? kBamItemBytes * item - a : 0;
    const uint64_t hi = kBamItemBytes * (item + 1) - a < size ? kBamItemBytes * (item + 1) - a : size;
    bam_emit_range(e, lo, hi, out + lo);
}

#ifndef VK_BAM_LANE_ONLY

constexpr uint32_t kBamEmitThreads = 256;

__device__ inline uint64_t bam_shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = __shfl_up(static_cast<uint32_t>(v), d, 64), hi = __shfl_up(static_cast<uint32_t>(v >> 32), d, 64);
    return static_cast<uint64_t>(hi) << 32 | lo;
}
__device__ inline uint64_t bam_shfl64(uint64_t v, uint32_t src) {
    const uint32_t lo = __shfl(static_cast<uint32_t>(v), static_cast<int>(src), 64);
    const uint32_t hi = __shfl(static_cast<uint32_t>(v >> 32), static_cast<int>(src), 64);
    return static_cast<uint64_t>(hi) << 32 | lo;
}
// Inclusive sum over the 64 lanes of a wavefront (all of them call it).
__device__ inline uint64_t bam_wave_incl_sum(uint64_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint64_t o = bam_shfl_up64(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// The files of a call (device arrays) and how they are cut.
struct BamMeta {
    const uint64_t *offs, *lens, *first;   // [nfiles]: the file in the buffer, its first record
    const uint64_t* seg_first;             // [nfiles + 1]: prefix sums of the files' segments (a file has at least one)
    const int32_t* n_ref;                  // [nfiles]
    uint32_t nfiles, seg_bytes;
};

// The streams of a call: stream s takes the reads `select[s]` of file `file[s]` into out_offs[s] .. + out_caps[s].
struct BamStreams {
    const uint32_t *file, *select;   // [nstreams]
    const uint64_t* seg_first;       // [nstreams + 1]: prefix sums of the streams' segments (those of their files)
    const uint64_t *out_offs, *out_caps;
    uint32_t nstreams;
};

struct BamSeg {
    uint64_t entry, exit;   // the record it is walked from; the first record at or past its end
    BamTally t;
    uint64_t base[3];       // per class: text bytes of the file's segments before this one (the link pass)
    uint32_t status, guessed;
    uint32_t nrec, pad;     // the records that start in it: their starts are noted
};

// What the link pass knows of a file.
struct BamFile {
    uint64_t recs[3], bytes[3];   // zero with a status
    uint32_t status, pad;
};

__device__ inline uint64_t bam_seg_end(const BamMeta& m, uint64_t len, uint64_t j) {
    const uint64_t e = (j + 1) * m.seg_bytes;
    return e < len ? e : len;
}

// The entry of `list` (n + 1 prefix sums, list[0] = 0, list[n] > g) that holds g.
__device__ inline uint32_t bam_locate(const uint64_t* list, uint32_t n, uint64_t g) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A wavefront per segment (the workgroup is one wavefront: blockIdx.x is the segment).
__global__ __launch_bounds__(64) void vk_bam_segment_kernel(const uint8_t* base, BamMeta m, uint32_t exclude, uint32_t flags, BamSeg* segs,
                                                            uint16_t* starts) {
    const uint64_t g = blockIdx.x;
    const uint32_t f = bam_locate(m.seg_first, m.nfiles, g);
    const uint64_t j = g - m.seg_first[f];
    const uint8_t* p = base + m.offs[f];
    const uint64_t len = m.lens[f];
    const uint64_t start = j * m.seg_bytes, end = bam_seg_end(m, len, j);
    const uint32_t lane = threadIdx.x;
    uint64_t entry = kBamNone;
    if (j == 0) {
        entry = m.first[f];
    } else if (!(flags & kBamNoGuess)) {
        const int32_t n_ref = m.n_ref[f];
        for (uint64_t c0 = start; c0 < end; c0 += 64) {   // (uniform: c0 and the ballot are the wavefront's)
            const uint64_t c = c0 + lane;
            const bool ok = c < end && bam_guess_ok(p, len, n_ref, c);
            const unsigned long long hit = __ballot(ok);
            if (hit) {
                entry = c0 + static_cast<uint32_t>(__ffsll(hit) - 1);
                break;
            }
        }
    }
    if (lane != 0) return;
    BamSeg& s = segs[g];
    s.entry = entry;
    s.guessed = entry != kBamNone ? 1u : 0u;
    BamTally t;
    uint64_t exit = entry;
    uint32_t st = 0, nrec = 0;
    const uint32_t cap = bam_starts_cap(m.seg_bytes);
    if (entry != kBamNone) st = bam_walk(p, len, entry, end, exclude, &t, &exit, start, starts + g * cap, cap, &nrec);
    else
        for (uint32_t c = 0; c < 3; ++c) t.recs[c] = t.bytes[c] = 0;
    s.exit = exit;
    s.t = t;
    s.status = st;
    s.nrec = nrec;
    s.pad = 0;
    for (uint32_t c = 0; c < 3; ++c) s.base[c] = 0;
}

// A wavefront per file.  link[0] += the file's segments, link[1] += those walked again.
__global__ __launch_bounds__(64) void vk_bam_link_kernel(const uint8_t* base, BamMeta m, uint32_t exclude, BamSeg* segs, uint16_t* starts,
                                                         BamFile* files, unsigned long long* link) {
    const uint32_t f = blockIdx.x;
    const uint64_t nseg = m.seg_first[f + 1] - m.seg_first[f];
    BamSeg* S = segs + m.seg_first[f];
    const uint8_t* p = base + m.offs[f];
    const uint64_t len = m.lens[f];
    const uint32_t lane = threadIdx.x;
    // (all of these are kept equal in every lane)
    uint64_t truth = m.first[f], carry_r[3] = {0, 0, 0}, carry_b[3] = {0, 0, 0}, rewalked = 0;
    uint32_t status = 0;
    uint64_t j0 = 0;
    while (j0 < nseg && status == 0) {
        const uint64_t j = j0 + lane;
        const bool valid = j < nseg;
        const uint64_t e = valid ? S[j].entry : kBamNone, x = valid ? S[j].exit : 0;
        const uint32_t guessed = valid ? S[j].guessed : 0u, st = valid ? S[j].status : 0u;
        uint64_t prev = bam_shfl_up64(x, 1);
        if (lane == 0) prev = truth;
        const unsigned long long ok = __ballot(valid && guessed && e == prev);
        const uint32_t n_ok = ~ok ? static_cast<uint32_t>(__ffsll(~ok) - 1) : 64u;   // the run of lanes whose entry is true
        if (n_ok) {
            const bool mine = lane < n_ok;
            const unsigned long long bad = __ballot(mine && st != 0);
            if (bad) {   // the first of them that met a bad record: the file has no text
                status = __shfl(st, __ffsll(bad) - 1, 64);
            } else {
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) {
                    const uint64_t b = mine ? S[j].t.bytes[c] : 0, r = mine ? S[j].t.recs[c] : 0;
                    const uint64_t ib = bam_wave_incl_sum(b), ir = bam_wave_incl_sum(r);
                    if (mine) S[j].base[c] = carry_b[c] + ib - b;
                    carry_b[c] += bam_shfl64(ib, 63);
                    carry_r[c] += bam_shfl64(ir, 63);
                }
                truth = bam_shfl64(x, n_ok - 1);
            }
            j0 += n_ok;
        } else {
            // segment j0 by lane 0: it starts no record, or it is walked from the true entry
            uint64_t exit = truth;
            uint32_t st1 = 0, walked = 0, nrec = 0;
            BamTally t;
            for (uint32_t c = 0; c < 3; ++c) t.recs[c] = t.bytes[c] = 0;
            if (lane == 0) {
                const uint64_t end = bam_seg_end(m, len, j0);
                if (truth < end) {
                    const uint32_t cap = bam_starts_cap(m.seg_bytes);
                    st1 = bam_walk(p, len, truth, end, exclude, &t, &exit, j0 * m.seg_bytes, starts + (m.seg_first[f] + j0) * cap, cap,
                                   &nrec);
                    walked = 1;
                }
                BamSeg& s = S[j0];
                s.entry = truth;
                s.exit = exit;
                s.t = t;
                s.status = st1;
                s.guessed = 1;
                s.nrec = nrec;
                for (uint32_t c = 0; c < 3; ++c) s.base[c] = carry_b[c];
            }
            status = __shfl(st1, 0, 64);
            rewalked += __shfl(walked, 0, 64);
            truth = bam_shfl64(exit, 0);
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                carry_b[c] += bam_shfl64(t.bytes[c], 0);
                carry_r[c] += bam_shfl64(t.recs[c], 0);
            }
            j0 += 1;
        }
        status = __builtin_amdgcn_readfirstlane(status);
    }
    if (lane != 0) return;
    if (status == 0 && truth != len) status = kBamTruncated;   // (a first_record behind the file's end)
    BamFile& o = files[f];
    for (uint32_t c = 0; c < 3; ++c) {
        o.recs[c] = status ? 0 : carry_r[c];
        o.bytes[c] = status ? 0 : carry_b[c];
    }
    o.status = status;
    o.pad = 0;
    atomicAdd(link, static_cast<unsigned long long>(nseg));
    atomicAdd(link + 1, static_cast<unsigned long long>(rewalked));
}

__device__ inline uint64_t bam_pick(const uint64_t* v, uint32_t select) { return select == kBamAll ? v[0] + v[1] + v[2] : v[select - 1]; }

// A workgroup per (stream, segment).  A file with a status, or a stream whose text does not fit its slot, is not written.
__global__ __launch_bounds__(kBamEmitThreads) void vk_bam_emit_kernel(const uint8_t* base, BamMeta m, BamStreams ss, uint32_t exclude,
                                                                      const BamSeg* segs, const uint16_t* starts, const BamFile* files,
                                                                      uint8_t* out) {
    __shared__ uint64_t s_pos[64], s_size[64], s_item0[65];
    __shared__ BamEmit s_e[64];
    __shared__ uint64_t s_bytes;
    const uint64_t g = blockIdx.x;
    const uint32_t s = bam_locate(ss.seg_first, ss.nstreams, g);
    const uint64_t j = g - ss.seg_first[s];
    const uint32_t f = ss.file[s], select = ss.select[s];
    if (files[f].status) return;
    const uint64_t cap = ss.out_caps[s];
    if (bam_pick(files[f].bytes, select) > cap) return;
    const BamSeg& sg = segs[m.seg_first[f] + j];
    const uint8_t* p = base + m.offs[f];
    const uint64_t len = m.lens[f], seg_start = j * m.seg_bytes;
    uint8_t* dst = out + ss.out_offs[s];
    uint64_t pos = bam_pick(sg.base, select);   // of the batch's first read in the stream's text
    const uint32_t scap = bam_starts_cap(m.seg_bytes);
    const uint32_t nrec = sg.nrec < scap ? sg.nrec : scap;
    const uint16_t* mine = starts + (m.seg_first[f] + j) * scap;
    for (uint32_t r0 = 0; r0 < nrec; r0 += 64) {   // (uniform: nrec is the workgroup's)
        if (threadIdx.x < 64) {   // a record per lane of the first wavefront: its read's place in the text, its items
            const uint32_t lane = threadIdx.x;
            uint64_t size = 0;
            BamEmit e{};
            BamRec r;
            if (r0 + lane < nrec && bam_read(p, len, seg_start + mine[r0 + lane], &r) == 0 &&
                bam_takes(select, bam_class(r, exclude))) {
                size = bam_text_size(r);
                e = bam_emit_of(p, r);
            }
            const uint64_t after = bam_wave_incl_sum(size);
            const uint64_t at = pos + after - size;
            if (at + size > cap) size = 0;   // (cannot be: the tallies are of these records)
            const uint64_t items = bam_items(dst + at, size);
            const uint64_t items_after = bam_wave_incl_sum(items);
            s_e[lane] = e;
            s_pos[lane] = at;
            s_size[lane] = size;
            s_item0[lane] = items_after - items;
            if (lane == 63) {
                s_item0[64] = items_after;
                s_bytes = after;
            }
        }
        __syncthreads();
        const uint64_t total = s_item0[64];
        for (uint64_t it = threadIdx.x; it < total; it += kBamEmitThreads) {
            uint32_t lo = 0, hi = 64;   // the last record whose items begin at or before `it`
#pragma unroll
            for (uint32_t step = 0; step < 6; ++step) {
                const uint32_t mid = (lo + hi) / 2;
                if (s_item0[mid] <= it) lo = mid;
                else hi = mid;
            }
            bam_emit_item(s_e[lo], dst + s_pos[lo], s_size[lo], it - s_item0[lo]);
        }
        pos += s_bytes;
        __syncthreads();
    }
}

#endif  // VK_BAM_LANE_ONLY

}  // namespace

#endif  // VK_BAM_H
