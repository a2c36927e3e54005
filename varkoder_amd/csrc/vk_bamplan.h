// vk_bamplan.h -- the host's side of the BAM conversion (vk_bam.h, vk_bam_groups.h): what a call carries, the rules its
// arguments must keep, the sizes and tables the host makes for the kernels, and what it makes of their results.  They run
// on caller input and are plain functions of a few integer arrays: no HIP here, so that a host compiler and a CPU test
// reach them (tests/emul/bamplan_emul.cpp, tests/emul/bam_groups_emul.cpp).
//
// The constants, bam_hash_step, bam_table_slots, bam_map_at and bam_starts_cap stay where the lanes use them: vkimg.hip
// includes this header behind vk_bam.h and vk_bam_groups.h; a host compiler gets their lane-local part through it.
#ifndef VK_BAMPLAN_H
#define VK_BAMPLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#ifndef VK_BAM_GROUPS_H
#ifndef __HIPCC__
#define __device__
#define __host__
#endif
#define VK_BAM_LANE_ONLY
#include "vk_bam.h"
#include "vk_bam_groups.h"
#endif
#include "vk_ws.h"

namespace {

// What a BAM call passes around, whichever of the four it is: the files, the streams, the groups of a grouped call (else
// null), the slots of a text call (else null).  The arrays are the caller's, on the host; d_bam and d_out are the device's.
struct BamCall {
    const uint8_t* d_bam;
    const uint64_t *offsets, *lengths, *first_record;   // [nfiles]
    const int32_t* n_ref;
    uint32_t nfiles;
    const uint32_t *group_first, *id_first;             // [nfiles + 1], [groups + 1]
    const uint8_t* id_bytes;
    const uint32_t *stream_file, *stream_select, *stream_group;   // [nstreams]
    uint32_t nstreams;
    uint8_t* d_out;
    const uint64_t *out_offsets, *out_caps;             // [nstreams]
    uint32_t exclude, flags;
    bool grouped, text;
};

// ---- the argument rules (the context and the device pointers are the callers' to check) ------------------------------

inline bool bam_args_ok(const BamCall& c) {
    if (c.flags & ~kBamNoGuess) return false;
    if (c.nfiles && (!c.offsets || !c.lengths || !c.first_record || !c.n_ref)) return false;
    if (c.nstreams && (!c.stream_file || !c.stream_select)) return false;
    for (uint32_t s = 0; s < c.nstreams; ++s)
        if (c.stream_file[s] >= c.nfiles || c.stream_select[s] > kBamSingle) return false;
    return true;
}

// Of a grouped call that bam_args_ok let pass.
inline bool bg_args_ok(const BamCall& c) {
    const uint32_t nfiles = c.nfiles;
    const uint32_t *group_first = c.group_first, *id_first = c.id_first;
    if (nfiles && (!group_first || !id_first || !c.lengths)) return false;
    if (c.nstreams && !c.stream_group) return false;
    if (nfiles && group_first[0] != 0) return false;
    for (uint32_t f = 0; f < nfiles; ++f)
        if (group_first[f + 1] < group_first[f] || group_first[f + 1] - group_first[f] > kBamMaxGroups) return false;
    const uint32_t tg = nfiles ? group_first[nfiles] : 0;
    if (tg && (!c.id_bytes || id_first[0] != 0)) return false;
    for (uint32_t g = 0; g < tg; ++g)
        if (id_first[g + 1] <= id_first[g] || id_first[g + 1] - id_first[g] > kBamMaxId) return false;
    for (uint32_t f = 0; f < nfiles; ++f) {   // an ID names one group of its file
        std::vector<std::string> ids;
        for (uint32_t g = group_first[f]; g < group_first[f + 1]; ++g)
            ids.emplace_back(reinterpret_cast<const char*>(c.id_bytes) + id_first[g], id_first[g + 1] - id_first[g]);
        std::sort(ids.begin(), ids.end());
        if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return false;
    }
    std::vector<uint8_t> kinds(nfiles, 0);   // 1: a stream of VK_BAM_ALL, 2: one of a class
    std::vector<std::pair<uint64_t, uint32_t>> keys;
    for (uint32_t s = 0; s < c.nstreams; ++s) {
        const uint32_t f = c.stream_file[s], g = c.stream_group[s];
        if (g != kBamUngrouped && g >= group_first[f + 1] - group_first[f]) return false;
        kinds[f] |= c.stream_select[s] == kBamAll ? 1 : 2;
        if (kinds[f] == 3) return false;
        keys.emplace_back(static_cast<uint64_t>(f) << 32 | g, c.stream_select[s]);
    }
    std::sort(keys.begin(), keys.end());
    return std::adjacent_find(keys.begin(), keys.end()) == keys.end();
}

// The segments of a file of `length` bytes: at least one.
inline uint64_t bam_file_segs(uint64_t length, uint32_t seg) {
    const uint64_t n = (length + seg - 1) / seg;
    return n ? n : 1;
}

// ---- the framing's plan -----------------------------------------------------------------------------------------------
// The streams are those of an ungrouped call: a grouped call's streams belong to its count pass, its framing has none.
struct BamPlan {
    uint32_t seg = 0, nstreams = 0;                 // bytes of a segment; streams of the framing
    std::vector<uint64_t> seg_first, sseg_first;    // [nfiles + 1], [nstreams + 1]: prefix sums of the segments
    std::vector<uint64_t> out_offs, out_caps;       // [nstreams]: the slots, zero when the call only frames
    uint64_t segs = 0, stream_segs = 0;
    bool ok = false;                                // false: 2^31 segments or stream segments, or more
};

inline BamPlan bam_plan(const BamCall& c, uint32_t seg_bytes) {
    BamPlan p;
    p.seg = seg_bytes ? seg_bytes : kBamSegBytes;
    p.nstreams = c.grouped ? 0 : c.nstreams;
    p.seg_first.assign(c.nfiles + 1ull, 0);
    for (uint32_t i = 0; i < c.nfiles; ++i) p.seg_first[i + 1] = p.seg_first[i] + bam_file_segs(c.lengths[i], p.seg);
    p.sseg_first.assign(p.nstreams + 1ull, 0);
    p.out_offs.assign(p.nstreams, 0);
    p.out_caps.assign(p.nstreams, 0);
    for (uint32_t s = 0; s < p.nstreams; ++s) {
        const uint32_t f = c.stream_file[s];
        p.sseg_first[s + 1] = p.sseg_first[s] + (p.seg_first[f + 1] - p.seg_first[f]);
        if (c.text) {
            p.out_offs[s] = c.out_offsets[s];
            p.out_caps[s] = c.out_caps[s];
        }
    }
    p.segs = p.seg_first[c.nfiles];
    p.stream_segs = p.sseg_first[p.nstreams];
    p.ok = p.segs < (1ull << 31) && p.stream_segs < (1ull << 31);
    return p;
}

// ---- a grouped call's plan --------------------------------------------------------------------------------------------

// What a grouped call's sizes come to: of its tables, its notes and its rows.
struct BgCounts {
    uint64_t groups = 0, id_bytes = 0, slots = 0, map = 0, segs = 0, scap = 0, panels = 0, rows = 0;
    uint32_t max_ls = 0;
    std::vector<uint32_t> nls;    // [nfiles]: a file's streams
    std::vector<uint64_t> npan;   // [nfiles]: a file's panels
};

inline BgCounts bg_counts(const BamCall& c, uint32_t seg, uint32_t panel) {
    BgCounts n;
    n.nls.assign(c.nfiles, 0);
    n.npan.assign(c.nfiles, 0);
    for (uint32_t s = 0; s < c.nstreams; ++s) n.nls[c.stream_file[s]] += 1;
    n.groups = c.nfiles ? c.group_first[c.nfiles] : 0;
    n.id_bytes = n.groups ? c.id_first[n.groups] : 0;
    n.scap = bam_starts_cap(seg);
    for (uint32_t f = 0; f < c.nfiles; ++f) {
        const uint32_t ng = c.group_first[f + 1] - c.group_first[f];
        n.slots += bam_table_slots(ng);
        n.map += 3ull * (ng + 1);
        const uint64_t nseg = bam_file_segs(c.lengths[f], seg);
        n.npan[f] = (nseg + panel - 1) / panel;
        n.segs += nseg;
        n.panels += n.npan[f];
        n.rows += n.npan[f] * n.nls[f];
        n.max_ls = std::max(n.max_ls, n.nls[f]);
    }
    return n;
}

// The descriptors (made on the host, uploaded as one block) and the device-only pieces of a grouped call.
struct BgPieces {
    uint8_t* ids;
    uint32_t *group_first, *id_first, *slots, *slot_first, *map_first, *ls_first, *ls_stream, *stream_file, *stream_local;
    uint16_t* map;
    uint64_t *pan_first, *row_first, *out_offs, *out_caps;
    size_t desc_bytes;
    uint32_t* aux_bad;
    unsigned long long* counters;   // aux_bad | counters: what a call reads back beside the totals, one run of bytes
    size_t back_bytes;
    uint16_t* notes;
    BamRow *rows, *totals;
};

// What the count pass reports beside the rows: one run of pieces, on the device and in the host's mirror of it.
inline void bg_back(WsTake& take, uint32_t*& aux_bad, unsigned long long*& counters, uint32_t nfiles) {
    take(aux_bad, nfiles);
    take(counters, 1);
}

// The pieces stated once: for the size (a taker without a base), for the host's block (its first desc_bytes), for the device.
inline void bg_take(WsTake& take, BgPieces& p, uint32_t nfiles, uint32_t nstreams, const BgCounts& n) {
    take(p.ids, n.id_bytes);
    take(p.group_first, nfiles + 1ull);
    take(p.id_first, n.groups + 1);
    take(p.slots, n.slots);
    take(p.slot_first, nfiles);
    take(p.map_first, nfiles);
    take(p.ls_first, nfiles + 1ull);
    take(p.ls_stream, nstreams);
    take(p.stream_file, nstreams);
    take(p.stream_local, nstreams);
    take(p.map, n.map);
    take(p.pan_first, nfiles + 1ull);
    take(p.row_first, nfiles);
    take(p.out_offs, nstreams);
    take(p.out_caps, nstreams);
    p.desc_bytes = take.at;
    bg_back(take, p.aux_bad, p.counters, nfiles);
    p.back_bytes = take.at - p.desc_bytes;
    take(p.notes, n.segs * n.scap);
    take(p.rows, n.rows);
    take(p.totals, nstreams);
}

// What vk_bam_groups_workspace_size states.
inline uint64_t bg_workspace_bytes(const BamCall& c, uint32_t seg, uint32_t panel) {
    WsTake size{nullptr, 0};
    BgPieces p{};
    bg_take(size, p, c.nfiles, c.nstreams, bg_counts(c, seg, panel));
    return size.at;
}

// The host's descriptor block of a grouped call that bg_args_ok let pass: `host` gets its desc_bytes, the pieces returned
// point into it.  Per file an open-addressed table of its IDs (slot = 1 + group; bam_probe reads it) and the map from
// (class, group) to the file's local stream (bam_map_at); per stream its file and its place among the file's streams.
inline BgPieces bg_describe(const BamCall& c, const BgCounts& n, std::vector<uint8_t>& host) {
    BgPieces h{};
    WsTake size{nullptr, 0};
    bg_take(size, h, c.nfiles, c.nstreams, n);
    host.assign(h.desc_bytes, 0);
    WsTake on_host{host.data(), 0};
    bg_take(on_host, h, c.nfiles, c.nstreams, n);
    if (n.id_bytes) memcpy(h.ids, c.id_bytes, n.id_bytes);
    memcpy(h.group_first, c.group_first, (c.nfiles + 1ull) * sizeof(uint32_t));
    if (n.groups) memcpy(h.id_first, c.id_first, (n.groups + 1) * sizeof(uint32_t));
    else h.id_first[0] = 0;
    uint32_t slot_at = 0, map_at = 0;
    uint64_t row_at = 0;
    h.ls_first[0] = 0;
    h.pan_first[0] = 0;
    for (uint32_t f = 0; f < c.nfiles; ++f) {
        const uint32_t g0 = c.group_first[f], ng = c.group_first[f + 1] - g0, nslots = bam_table_slots(ng);
        h.slot_first[f] = slot_at;
        for (uint32_t g = 0; g < ng; ++g) {
            uint32_t hash = kBamHashSeed;
            for (uint32_t i = c.id_first[g0 + g]; i < c.id_first[g0 + g + 1]; ++i) hash = bam_hash_step(hash, c.id_bytes[i]);
            uint32_t i = hash & (nslots - 1);
            while (h.slots[slot_at + i]) i = (i + 1) & (nslots - 1);
            h.slots[slot_at + i] = g + 1;
        }
        slot_at += nslots;
        h.map_first[f] = map_at;
        for (uint32_t i = 0; i < 3 * (ng + 1); ++i) h.map[map_at + i] = kBamNoStream;
        map_at += 3 * (ng + 1);
        h.ls_first[f + 1] = h.ls_first[f] + n.nls[f];
        h.pan_first[f + 1] = h.pan_first[f] + n.npan[f];
        h.row_first[f] = row_at;
        row_at += n.npan[f] * n.nls[f];
    }
    std::vector<uint32_t> seen(c.nfiles, 0);
    for (uint32_t s = 0; s < c.nstreams; ++s) {
        const uint32_t f = c.stream_file[s], ng = c.group_first[f + 1] - c.group_first[f], local = seen[f]++;
        h.stream_file[s] = f;
        h.stream_local[s] = local;
        h.ls_stream[h.ls_first[f] + local] = s;
        uint16_t* map = h.map + h.map_first[f];
        for (uint32_t cls = 1; cls <= 3; ++cls)
            if (c.stream_select[s] == kBamAll || c.stream_select[s] == cls)
                map[bam_map_at(cls, c.stream_group[s], ng)] = static_cast<uint16_t>(local);
        h.out_offs[s] = c.text ? c.out_offsets[s] : 0;
        h.out_caps[s] = c.text ? c.out_caps[s] : 0;
    }
    return h;
}

// ---- the result rules ---------------------------------------------------------------------------------------------------

// Of a file's per-class figures v[3], what a stream of `select` takes.
inline uint64_t bam_host_pick(const uint64_t* v, uint32_t select) { return select == kBamAll ? v[0] + v[1] + v[2] : v[select - 1]; }

// A file's status: its own, else VK_BAM_BAD_AUX when an aux area of it did not parse (a grouped call).
inline uint32_t bam_status_of(uint32_t file_status, uint32_t aux_bad) { return file_status ? file_status : aux_bad ? kBamBadAux : 0u; }

// A stream's text of n bytes and its slot of cap bytes: *length = n when it fits, else 0 and false (VK_ENOSPC).
inline bool bam_slot_fits(uint64_t n, uint64_t cap, uint64_t* length) {
    *length = n <= cap ? n : 0;
    return n <= cap;
}

}  // namespace

#endif  // VK_BAMPLAN_H
