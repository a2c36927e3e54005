// vk_bam_groups.h -- a BAM file's reads split by read group: `image / query --from-bam --bam-read-groups`
// (vk_bam_groups_frame_device, vk_bam_groups_fastq_device).  Part of the one translation unit vkimg.hip, behind vk_bam.h.
//
// The rule ("--from-bam --bam-read-groups: the rule"; tests/bam_groups_ref.py is the same rule in Python): a
// file's groups are the IDs of its header's @RG lines; a read's group is the one whose ID equals the value of the first `RG`
// field of its aux area (type Z), and a read without one is ungrouped (VK_BAM_UNGROUPED).  A stream takes the reads of one
// (file, select, group); a read goes to at most one stream.
//
// The framing is vk_bam.h's as it is: once its link pass is through, every noted start is a true record.  Behind it:
//     vk_bam_groups_count_kernel   a workgroup per PANEL of kBamPanelSegs (4) consecutive segments, a lane per record: the lane
//                                  walks the record's aux fields (every length checked against the block's end before it is
//                                  followed), hashes the RG value, probes the file's open-addressed table (built on the
//                                  host) and compares bytes; it notes the record's stream (a u16 among the file's streams,
//                                  or none) beside the record's start and adds the read and its text bytes to the stream's
//                                  entry of a table in LDS.  The table goes out as the panel's ROW
//     vk_bam_groups_scan_kernel    a wavefront per stream runs down its file's rows, 64 at a step: every row's entry becomes
//                                  the place in the stream's text where the panel's reads begin; the totals go to the stream
//     vk_bam_groups_emit_kernel    a workgroup per panel, however many streams there are: the row is loaded into LDS as
//                                  the streams' cursors; the records are taken 64 at a time in order, a read's place is its
//                                  stream's cursor plus the sizes of the earlier lanes of the same stream, and the last
//                                  lane of every stream moves the cursor on (one wavefront, in order: no atomic decides a
//                                  place).  The bytes are written by bam_emit_item, as in vk_bam_emit_kernel
// A file's records are read twice (count, emit), once each, whatever the number of groups.
//
// The lane-local code -- a field's size, the walk, hash, probe and compare -- compiles for the host under
// VK_BAM_LANE_ONLY: tests/emul/bam_groups_emul.cpp.
#ifndef VK_BAM_GROUPS_H
#define VK_BAM_GROUPS_H

namespace {

constexpr uint32_t kBamBadAux = 3;                 // VK_BAM_BAD_AUX
constexpr uint32_t kBamUngrouped = 0xFFFFFFFFu;    // VK_BAM_UNGROUPED
constexpr uint32_t kBamMaxGroups = 1024;           // VK_BAM_MAX_GROUPS
constexpr uint32_t kBamMaxId = 255;                // bytes of an ID
constexpr uint32_t kBamPanelSegs = 4;              // segments of a panel (VKIMG_BAM_PANEL_SEGS)
constexpr uint16_t kBamNoStream = 0xFFFF;          // a record's note: no stream takes it
constexpr uint32_t kBamAuxBad = 0xFFFFFFFEu;       // bam_group_of: the aux area does not parse

// FNV-1a over an ID's (a value's) bytes: the host builds a file's table with it, the lanes probe with it.
__host__ __device__ inline uint32_t bam_hash_step(uint32_t h, uint8_t b) { return (h ^ b) * 16777619u; }
constexpr uint32_t kBamHashSeed = 2166136261u;

// A file's groups as the lanes see them.
struct BamGroupTable {
    const uint8_t* ids;         // the call's ID bytes
    const uint32_t* id_first;   // [ngroups + 1]: this file's IDs in `ids`
    const uint32_t* slots;      // [mask + 1]: 0, or 1 + the group whose ID hashes there (open addressing, linear probing)
    uint32_t mask, ngroups;
};

// The slots a table of n groups has: a power of two, at least 2 n (so a probe ends at an empty slot).
__host__ __device__ inline uint32_t bam_table_slots(uint32_t n) {
    uint32_t s = 2;
    while (s < 2 * n) s <<= 1;
    return s;
}

// Bytes of a value of fixed size by its type; 0: not such a type.
__device__ inline uint32_t bam_aux_fixed(uint8_t type) {
    switch (type) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
    }
}
// Bytes of an element of a B array by its subtype; 0: not one.
__device__ inline uint32_t bam_aux_elem(uint8_t sub) { return sub == 'A' ? 0 : bam_aux_fixed(sub); }

// The group whose ID is the n bytes at v; kBamUngrouped without one.
__device__ inline uint32_t bam_probe(const BamGroupTable& T, const uint8_t* v, uint32_t n, uint32_t hash) {
    if (T.ngroups == 0) return kBamUngrouped;
    for (uint32_t i = hash & T.mask;; i = (i + 1) & T.mask) {
        const uint32_t e = T.slots[i];
        if (e == 0) return kBamUngrouped;
        const uint32_t g = e - 1, a = T.id_first[g];
        if (T.id_first[g + 1] - a != n) continue;
        uint32_t k = 0;
        while (k < n && T.ids[a + k] == v[k]) ++k;
        if (k == n) return g;
    }
}

// The group of the read whose block is blk[0 .. bs) and whose aux fields begin at `at` (<= bs): an index into the file's
// table, kBamUngrouped, or kBamAuxBad.  Nothing at or past blk + bs is read.
__device__ inline uint32_t bam_group_of(const uint8_t* blk, uint64_t bs, uint64_t at, const BamGroupTable& T) {
    while (at < bs) {
        if (bs - at < 3) return kBamAuxBad;
        const uint8_t t0 = blk[at], t1 = blk[at + 1], type = blk[at + 2];
        at += 3;
        if (t0 == 'R' && t1 == 'G') {   // the deciding field: nothing behind it is looked at
            if (type != 'Z') return kBamUngrouped;
            uint32_t h = kBamHashSeed, n = 0;
            while (at + n < bs && blk[at + n] != 0 && n <= kBamMaxId) h = bam_hash_step(h, blk[at + n++]);
            if (at + n >= bs || n > kBamMaxId) return kBamUngrouped;   // no NUL in the block, or longer than any ID
            return bam_probe(T, blk + at, n, h);
        }
        const uint32_t fixed = bam_aux_fixed(type);
        if (fixed) {
            if (bs - at < fixed) return kBamAuxBad;
            at += fixed;
        } else if (type == 'Z' || type == 'H') {
            while (at < bs && blk[at] != 0) ++at;
            if (at >= bs) return kBamAuxBad;
            at += 1;
        } else if (type == 'B') {
            if (bs - at < 5) return kBamAuxBad;
            const uint64_t elem = bam_aux_elem(blk[at]), count = bam_u32(blk + at + 1);
            at += 5;
            if (elem == 0 || bs - at < elem * count) return kBamAuxBad;
            at += elem * count;
        } else {
            return kBamAuxBad;
        }
    }
    return kBamUngrouped;
}

// Where the aux fields of a record that bam_read let pass begin, within its block.
__device__ inline uint64_t bam_aux_at(const BamRec& r) {
    return 32ull + r.l_name + 4ull * r.n_cigar + (static_cast<uint64_t>(r.l_seq) + 1) / 2 + r.l_seq;
}

// A file's map from (class, group) to the stream that takes such a read: map[(cls - 1) * (ngroups + 1) + slot], slot = the
// group, or ngroups for an ungrouped read; kBamNoStream: none.
__host__ __device__ inline uint32_t bam_map_at(uint32_t cls, uint32_t group, uint32_t ngroups) {
    return (cls - 1) * (ngroups + 1) + (group == kBamUngrouped ? ngroups : group);
}

// The note of the record r (of class cls != 0): its stream among the file's, kBamNoStream, or -- *bad = 1 -- an aux area
// that does not parse.
__device__ inline uint16_t bam_note_of(const uint8_t* p, const BamRec& r, uint32_t cls, const BamGroupTable& T, const uint16_t* map,
                                       uint32_t* bad) {
    const uint32_t g = bam_group_of(p + r.at + 4, r.block_size, bam_aux_at(r), T);
    if (g == kBamAuxBad) {
        *bad = 1;
        return kBamNoStream;
    }
    return map[bam_map_at(cls, g, T.ngroups)];
}

struct BamRow {
    uint64_t recs, bytes;   // of a panel's reads in one stream; behind the scan `bytes` is where they begin in its text
};

#ifndef VK_BAM_LANE_ONLY

constexpr uint32_t kBamCountThreads = 256;

// The groups and streams of a call's files (device arrays), on top of BamMeta.
struct BamGroupsMeta {
    const uint8_t* ids;
    const uint32_t* group_first;   // [nfiles + 1]
    const uint32_t* id_first;      // [total groups + 1]
    const uint32_t* slots;         // every file's table, one after another
    const uint32_t* slot_first;    // [nfiles]: a file's table in `slots`
    const uint16_t* map;           // every file's (class, group) map
    const uint32_t* map_first;     // [nfiles]
    const uint32_t* ls_first;      // [nfiles + 1]: prefix sums of the files' streams (local streams)
    const uint32_t* ls_stream;     // [nstreams]: the call's stream of a file's local stream
    const uint64_t* pan_first;     // [nfiles + 1]: prefix sums of the files' panels
    const uint64_t* row_first;     // [nfiles]: a file's first row entry in the rows
    uint32_t panel_segs;
};

__device__ inline BamGroupTable bam_table_of(const BamGroupsMeta& G, uint32_t f) {
    const uint32_t g0 = G.group_first[f], n = G.group_first[f + 1] - g0;
    return BamGroupTable{G.ids, G.id_first + g0, G.slots + G.slot_first[f], bam_table_slots(n) - 1, n};
}

// A workgroup per panel; dynamic LDS: a BamRow per stream of the file.  aux_bad[f] = 1 for a file with an aux area that does
// not parse; counters[0] += the records whose aux was walked.
__global__ __launch_bounds__(kBamCountThreads) void vk_bam_groups_count_kernel(const uint8_t* base, BamMeta m, BamGroupsMeta G,
                                                                              uint32_t exclude, const BamSeg* segs,
                                                                              const uint16_t* starts, const BamFile* files,
                                                                              uint16_t* notes, BamRow* rows, uint32_t* aux_bad,
                                                                              unsigned long long* counters) {
    extern __shared__ __align__(16) unsigned long long s_tab[];   // [2 * nls]: recs, bytes
    __shared__ uint32_t s_walked;
    const uint64_t g = blockIdx.x;
    const uint32_t f = bam_locate(G.pan_first, m.nfiles, g);
    if (files[f].status) return;   // (its starts are not all noted; its streams get nothing)
    const uint64_t pan = g - G.pan_first[f];
    const uint32_t nls = G.ls_first[f + 1] - G.ls_first[f];
    for (uint32_t i = threadIdx.x; i < 2 * nls; i += kBamCountThreads) s_tab[i] = 0;
    if (threadIdx.x == 0) s_walked = 0;
    __syncthreads();
    const BamGroupTable T = bam_table_of(G, f);
    const uint16_t* map = G.map + G.map_first[f];
    const uint8_t* p = base + m.offs[f];
    const uint64_t len = m.lens[f];
    const uint64_t nseg = m.seg_first[f + 1] - m.seg_first[f];
    const uint64_t j0 = pan * G.panel_segs, j1 = j0 + G.panel_segs < nseg ? j0 + G.panel_segs : nseg;
    const uint32_t scap = bam_starts_cap(m.seg_bytes);
    uint32_t walked = 0, bad = 0;
    for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t sg = m.seg_first[f] + j;
        const uint32_t nrec = segs[sg].nrec < scap ? segs[sg].nrec : scap;
        for (uint32_t i = threadIdx.x; i < nrec; i += kBamCountThreads) {
            BamRec r;
            uint16_t note = kBamNoStream;
            if (bam_read(p, len, j * m.seg_bytes + starts[sg * scap + i], &r) == 0) {
                const uint32_t cls = bam_class(r, exclude);
                if (cls) {
                    note = bam_note_of(p, r, cls, T, map, &bad);
                    ++walked;
                    if (note != kBamNoStream) {
                        atomicAdd(&s_tab[2u * note], 1ull);
                        atomicAdd(&s_tab[2u * note + 1], static_cast<unsigned long long>(bam_text_size(r)));
                    }
                }
            }
            notes[sg * scap + i] = note;
        }
    }
    if (walked) atomicAdd(&s_walked, walked);
    if (bad) aux_bad[f] = 1;
    __syncthreads();
    BamRow* row = rows + G.row_first[f] + pan * nls;
    for (uint32_t i = threadIdx.x; i < nls; i += kBamCountThreads) row[i] = BamRow{s_tab[2 * i], s_tab[2 * i + 1]};
    if (threadIdx.x == 0 && s_walked) atomicAdd(counters, static_cast<unsigned long long>(s_walked));
}

// A wavefront per stream of the call (four to a workgroup), 64 of its file's rows at a step: a wave prefix sum gives every row
// its place.  totals[s] = the stream's reads and bytes (zero for a file with a status).
__global__ __launch_bounds__(256) void vk_bam_groups_scan_kernel(BamMeta m, BamGroupsMeta G, const uint32_t* stream_file,
                                                                 const uint32_t* stream_local, uint32_t nstreams, const BamFile* files,
                                                                 const uint32_t* aux_bad, BamRow* rows, BamRow* totals) {
    // (the stream is the wavefront's: said to the compiler, so that the loop below is left by a scalar branch and its
    // shuffles run with every lane -- tools/asm_lint.py, convergence)
    const uint32_t s = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64), lane = threadIdx.x & 63u;
    if (s >= nstreams) return;   // (the whole wavefront)
    const uint32_t f = stream_file[s], l = stream_local[s];
    uint64_t recs = 0, bytes = 0;   // (equal in every lane)
    if (files[f].status == 0 && aux_bad[f] == 0) {
        const uint32_t nls = G.ls_first[f + 1] - G.ls_first[f];
        const uint32_t npan = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(G.pan_first[f + 1] - G.pan_first[f]));
        BamRow* mine = rows + G.row_first[f] + l;
        for (uint32_t p0 = 0; p0 < npan; p0 += 64) {   // (uniform)
            const uint64_t p = static_cast<uint64_t>(p0) + lane;
            BamRow here{0, 0};
            if (p < npan) here = mine[p * nls];
            const uint64_t ib = bam_wave_incl_sum(here.bytes), ir = bam_wave_incl_sum(here.recs);
            if (p < npan) mine[p * nls].bytes = bytes + ib - here.bytes;
            bytes += bam_shfl64(ib, 63);
            recs += bam_shfl64(ir, 63);
        }
    }
    if (lane == 0) totals[s] = BamRow{recs, bytes};
}

constexpr uint64_t kBamNoCursor = ~0ull;   // a stream whose text does not fit its slot

// A workgroup per panel; dynamic LDS: a cursor (u64, a place in `out`) per stream of the file.
__global__ __launch_bounds__(kBamEmitThreads) void vk_bam_groups_emit_kernel(const uint8_t* base, BamMeta m, BamGroupsMeta G,
                                                                            const uint64_t* out_offs, const uint64_t* out_caps,
                                                                            const BamSeg* segs, const uint16_t* starts,
                                                                            const uint16_t* notes, const BamFile* files,
                                                                            const uint32_t* aux_bad, const BamRow* rows,
                                                                            const BamRow* totals, uint8_t* out) {
    extern __shared__ __align__(16) unsigned long long s_cursor[];   // [nls]
    __shared__ uint64_t s_pos[64], s_size[64], s_item0[65];
    __shared__ BamEmit s_e[64];
    const uint64_t g = blockIdx.x;
    const uint32_t f = bam_locate(G.pan_first, m.nfiles, g);
    if (files[f].status || aux_bad[f]) return;
    const uint64_t pan = g - G.pan_first[f];
    const uint32_t ls0 = G.ls_first[f], nls = G.ls_first[f + 1] - ls0;
    if (nls == 0) return;
    const BamRow* row = rows + G.row_first[f] + pan * nls;
    for (uint32_t i = threadIdx.x; i < nls; i += kBamEmitThreads) {
        const uint32_t s = G.ls_stream[ls0 + i];
        s_cursor[i] = totals[s].bytes <= out_caps[s] ? out_offs[s] + row[i].bytes : kBamNoCursor;
    }
    __syncthreads();
    const uint8_t* p = base + m.offs[f];
    const uint64_t len = m.lens[f];
    const uint64_t nseg = m.seg_first[f + 1] - m.seg_first[f];
    const uint64_t j0 = pan * G.panel_segs, j1 = j0 + G.panel_segs < nseg ? j0 + G.panel_segs : nseg;
    const uint32_t scap = bam_starts_cap(m.seg_bytes);
    for (uint64_t j = j0; j < j1; ++j) {   // (uniform: the bounds are the workgroup's)
        const uint64_t sg = m.seg_first[f] + j;
        const uint32_t nrec = segs[sg].nrec < scap ? segs[sg].nrec : scap;
        for (uint32_t r0 = 0; r0 < nrec; r0 += 64) {
            if (threadIdx.x < 64) {   // a record per lane of the first wavefront
                const uint32_t lane = threadIdx.x;
                uint64_t size = 0, cursor = kBamNoCursor;
                uint32_t note = kBamNoStream;
                BamEmit e{};
                BamRec r;
                if (r0 + lane < nrec) note = notes[sg * scap + r0 + lane];
                if (note < nls) cursor = s_cursor[note];
                else note = kBamNoStream;
                if (cursor != kBamNoCursor && bam_read(p, len, j * m.seg_bytes + starts[sg * scap + r0 + lane], &r) == 0) {
                    size = bam_text_size(r);
                    e = bam_emit_of(p, r);
                } else {
                    note = kBamNoStream;
                }
                // the sizes of the earlier lanes of the same stream; whether a later lane has it
                uint64_t before = 0;
                bool last = true;
                for (uint32_t k = 0; k < 64; ++k) {
                    const uint32_t nk = __shfl(note, static_cast<int>(k), 64);
                    const uint64_t zk = bam_shfl64(size, k);
                    if (nk == note && k < lane) before += zk;
                    if (nk == note && k > lane) last = false;
                }
                const uint64_t at = note != kBamNoStream ? cursor + before : 0;
                if (note != kBamNoStream && last) s_cursor[note] = at + size;
                const uint64_t items = bam_items(out + at, size);
                const uint64_t items_after = bam_wave_incl_sum(items);
                s_e[lane] = e;
                s_pos[lane] = at;
                s_size[lane] = size;
                s_item0[lane] = items_after - items;
                if (lane == 63) s_item0[64] = items_after;
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
                bam_emit_item(s_e[lo], out + s_pos[lo], s_size[lo], it - s_item0[lo]);
            }
            __syncthreads();
        }
    }
}

#endif  // VK_BAM_LANE_ONLY

}  // namespace

#endif  // VK_BAM_GROUPS_H
