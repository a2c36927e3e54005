// vk_textplan.h -- the host's side of the calls that work on record text in HBM: vk_ladder_emit_device (vk_emit.h),
// vk_screen_build_device and vk_screen_device (vk_screen.h), vk_spectrum_device (vk_spectrum.h), vk_spectrum_fasta_device
// (vk_fasta_spectrum.h), vk_depth_device (vk_depth.h) and vk_qc_device (vk_qc.h).  What a call carries, the rules its
// arguments must keep, the record index of a batch whose samples are one file each, the launch grids and the pieces of
// the workspaces.  They run on caller input and are plain functions of a few integer arrays: no HIP here, so that a host
// compiler and a CPU test reach them (tests/emul/textplan_emul.cpp).
//
// The constants and the plain structs stay where the kernels use them: vkimg.hip includes this header behind the device
// headers; a host compiler gets their plain part through it (VK_TEXT_STRUCTS_ONLY, the *_LANE_ONLY fences) and states
// itself the two atomics that vk_spectrum.h's lane code names.
//
// A known wart, kept: an output region smaller than its sample is VK_ENOSPC from vk_screen_device and VK_EINVAL from
// vk_depth_device (kScreenRules, kDepthRules).  Callers may tell the two apart, so it is written down here, not fixed.
#ifndef VK_TEXTPLAN_H
#define VK_TEXTPLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "vkimg.h"
#ifndef VK_SPECTRUM_H
#ifndef __HIPCC__
#define __device__
#define __host__
#endif
#define VK_TEXT_STRUCTS_ONLY
#define VK_FASTA_LANE_ONLY
#define VK_SCREEN_LANE_ONLY
#define VK_SPECTRUM_LANE_ONLY
#include "vk_clean.h"
#include "vk_emit.h"
#include "vk_fasta.h"
#include "vk_spectrum.h"
#endif
#include "vk_faplan.h"
#include "vk_ws.h"

namespace {

// What a call on record text passes around, whichever it is; a call leaves what it does not have at null or 0.  The arrays
// are the caller's, on the host, one entry per sample (a stream of vk_qc_device, an assembly of vk_spectrum_fasta_device).
struct TextCall {
    const uint64_t *offsets, *lengths, *records;
    uint32_t nsamples;
    const uint64_t *nslots, *slot_base;   // the samples' counting tables
    const uint64_t* out_offsets;          // the samples' regions of the kept text
    uint64_t out_capacity;
    const uint32_t *lo, *hi;              // the samples' depth bands
    int k;
    uint32_t every, min_hits;
};

// ---- the argument rules (the context, the null pointers and the workspace's size are the entry points' to check) -------

inline bool sc_slots_ok(uint64_t nslots) { return nslots >= kScMinSlots && nslots <= (1ull << 40) && (nslots & (nslots - 1)) == 0; }
inline bool text_k_ok(int k) { return k >= static_cast<int>(kScMinK) && k <= static_cast<int>(kScMaxK); }
inline bool text_grid_ok(uint64_t blocks) { return blocks < (1ull << 31); }   // (a grid's x is 31 bits)

// What differs between the calls in the rules of a sample.
struct TextRules {
    uint64_t max_length;   // a sample's bytes at most
    bool tables, bands;    // nslots[i] sizes a table; lo[i] <= hi[i]
    int short_region;      // the status of an output region smaller than its sample (0: the call writes no text)
};
// a multiplicity is 32-bit (2^33); the lanes' sums and a record's lengths are 32-bit (below 2^32); the screen and the emit
// path hold nothing that a long sample overflows
constexpr TextRules kEmitRules{~0ull, false, false, 0};
constexpr TextRules kScreenRules{~0ull, false, false, VK_ENOSPC};
constexpr TextRules kSpectrumRules{1ull << 33, true, false, 0};
constexpr TextRules kDepthRules{1ull << 33, true, true, VK_EINVAL};
constexpr TextRules kQcRules{(1ull << 32) - 1, false, false, 0};

// The samples one after another, each against its rules in this order: a text at a multiple of 16 bytes (and so its
// region), its length, its table, its band: VK_EINVAL; then a region as large as the sample's input inside the output:
// r.short_region.  The first sample that breaks a rule decides.
inline int text_samples_check(const TextCall& c, const TextRules& r) {
    for (uint32_t i = 0; i < c.nsamples; ++i) {
        if (c.offsets[i] % 16 || c.lengths[i] > r.max_length) return VK_EINVAL;
        if (r.short_region && c.out_offsets[i] % 16) return VK_EINVAL;
        if (r.tables && !sc_slots_ok(c.nslots[i])) return VK_EINVAL;
        if (r.bands && c.lo[i] > c.hi[i]) return VK_EINVAL;
        if (r.short_region &&
            (c.out_offsets[i] > c.out_capacity || (c.lengths[i] + 15) / 16 * 16 > c.out_capacity - c.out_offsets[i]))
            return r.short_region;
    }
    return VK_OK;
}

// Workgroups that take `per` items each, sample by sample: base[i] the first of sample i, base[n] all of them.  False when
// they are more than a grid holds.  (The tables' init and histogram kernels at kSpSlotsPerBlock slots, vk_qc_count_kernel
// at its records per workgroup.)
inline bool text_blocks(const uint64_t* items, uint32_t n, uint64_t per, std::vector<uint64_t>* base) {
    base->assign(n + 1ull, 0);
    for (uint32_t i = 0; i < n; ++i) (*base)[i + 1] = (*base)[i] + (items[i] + per - 1) / per;
    return text_grid_ok((*base)[n]);
}

inline uint64_t text_records(const uint64_t* records, uint32_t nsamples) {   // the records of the batch
    uint64_t nrec = 0;
    for (uint32_t i = 0; i < nsamples; ++i) nrec += records[i];
    return nrec;
}

// the workgroups of a kernel that takes kScRecsPerBlock records of the batch at a time (match, write, count)
inline uint64_t text_record_blocks(uint64_t nrec) { return (nrec + kScRecsPerBlock - 1) / kScRecsPerBlock; }

// The calls' rules, each in the order its entry point has always applied them (all but the screen's short region give
// VK_EINVAL, so only there does the order show: sample i's short region comes before sample i + 1's misaligned text).

inline int emit_check(const TextCall& c, const uint32_t* step_sample, const uint64_t* step_threshold, uint32_t nsteps) {
    if (int rc = text_samples_check(c, kEmitRules)) return rc;
    for (uint32_t j = 0; j < nsteps; ++j)
        if (step_sample[j] >= c.nsamples || step_threshold[j] > (1ull << 32)) return VK_EINVAL;
    return VK_OK;
}

inline int screen_build_check(uint64_t length, int k, bool table, uint64_t nslots) {
    if (length > VK_SCREEN_MAX_REF || !text_k_ok(k)) return VK_EINVAL;
    return table != (nslots != 0) || (table && !sc_slots_ok(nslots)) ? VK_EINVAL : VK_OK;
}

inline int screen_check(const TextCall& c, uint64_t table_slots) {
    if (!text_k_ok(c.k) || c.min_hits < 1 || !sc_slots_ok(table_slots)) return VK_EINVAL;
    return text_samples_check(c, kScreenRules);
}

// block_base: the table plan (text_blocks of nslots at kSpSlotsPerBlock).  Without records (FASTA) no record kernel runs.
inline int spectrum_check(const TextCall& c, std::vector<uint64_t>* block_base) {
    if (!text_k_ok(c.k) || c.every < 1) return VK_EINVAL;
    if (int rc = text_samples_check(c, kSpectrumRules)) return rc;
    if (!text_blocks(c.nslots, c.nsamples, kSpSlotsPerBlock, block_base)) return VK_EINVAL;
    return c.records && !text_grid_ok(text_record_blocks(text_records(c.records, c.nsamples))) ? VK_EINVAL : VK_OK;
}

inline int depth_check(const TextCall& c) {
    if (!text_k_ok(c.k) || c.every < 1) return VK_EINVAL;
    if (int rc = text_samples_check(c, kDepthRules)) return rc;
    return text_grid_ok(text_record_blocks(text_records(c.records, c.nsamples))) ? VK_OK : VK_EINVAL;
}

inline int qc_check(const TextCall& c, uint32_t per_block, std::vector<uint64_t>* block_base) {
    if (int rc = text_samples_check(c, kQcRules)) return rc;
    return text_blocks(c.records, c.nsamples, per_block, block_base) ? VK_OK : VK_EINVAL;
}

// ---- the record index (vk_clean.h's newline passes fill it: cl_index_run in vkimg.hip) -----------------------------------

inline uint32_t cl_rank(uint32_t role) { return role == VK_CL_ROLE_UNPAIRED ? 2u : role - 1u; }   // a file's group: R1, R2, single reads

// the files in the library's order: by sample, then R1, R2, unpaired, each in the caller's order (no roles: the caller's)
inline std::vector<uint32_t> cl_order(const uint32_t* roles, const uint32_t* samples, uint32_t nfiles) {
    std::vector<uint32_t> order(nfiles);
    for (uint32_t i = 0; i < nfiles; ++i) order[i] = i;
    if (roles)
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return samples[a] != samples[b] ? samples[a] < samples[b] : cl_rank(roles[a]) < cl_rank(roles[b]);
        });
    return order;
}

// The record index of a launch as the host states it: the file tables that the kernels read and, per group
// (3 * sample + cl_rank), the ordinal of its first record and the records it gives.
struct ClIndex {
    std::vector<ClFile> files;
    std::vector<uint64_t> fchunk, first, count;
    uint64_t nchunks = 0, nrec = 0;
};

// A file gives its budget records[i], the files of a group no more than group_cap between them (detection's evaluation
// set: a group's first kAdEval records, in the order of its files).  Without records (vk_clean_lines_device) the files
// stay in the caller's order and nothing is indexed.
inline ClIndex cl_index(const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records, const uint32_t* roles,
                        const uint32_t* samples, uint32_t nfiles, uint32_t nsamples, uint64_t group_cap) {
    ClIndex ix;
    ix.files.resize(nfiles);
    ix.fchunk.resize(nfiles);
    ix.first.assign(3ull * nsamples, 0);
    ix.count.assign(3ull * nsamples, 0);
    const std::vector<uint32_t> order = cl_order(roles, samples, nfiles);
    for (uint32_t j = 0; j < nfiles; ++j) {
        const uint32_t i = order[j];
        uint64_t n = 0;
        if (records) {
            const uint64_t g = 3ull * samples[i] + cl_rank(roles[i]);
            n = std::min(records[i], group_cap - ix.count[g]);
            // (a group's files are adjacent and those ahead of its first record give none, so this is the ordinal at the
            // group's first file as well; a group without files keeps 0)
            if (ix.count[g] == 0) ix.first[g] = ix.nrec;
            ix.count[g] += n;
        }
        ix.files[j] = ClFile{offsets[i], lengths[i], n, ix.nrec, ix.nchunks};
        ix.fchunk[j] = ix.nchunks;
        ix.nchunks += (lengths[i] + kClChunk - 1) / kClChunk;
        ix.nrec += n;
    }
    return ix;
}

// The index of a batch whose samples are one file each, as every call here takes its text: the index, the samples' rows
// for the kernels, and rec_base, the ordinal of a sample's first record (rec_base[n]: the records of the batch).
struct TextIndex {
    ClIndex ix;
    std::vector<EmSample> rows;
    std::vector<uint64_t> rec_base;
};

inline TextIndex text_index(const uint64_t* offsets, const uint64_t* lengths, const uint64_t* records, uint32_t nsamples) {
    TextIndex t;
    std::vector<uint32_t> roles(nsamples, VK_CL_ROLE_UNPAIRED), owner(nsamples);
    for (uint32_t i = 0; i < nsamples; ++i) owner[i] = i;
    t.ix = cl_index(offsets, lengths, records, roles.data(), owner.data(), nsamples, nsamples, ~0ull);
    t.rows.resize(nsamples);
    t.rec_base.assign(nsamples + 1ull, 0);
    for (uint32_t i = 0; i < nsamples; ++i) {
        t.rows[i] = EmSample{offsets[i], lengths[i], t.ix.files[i].rec0, t.ix.files[i].nrec, t.ix.files[i].chunk0,
                             i + 1 < nsamples ? t.ix.files[i + 1].chunk0 : t.ix.nchunks};
        t.rec_base[i + 1] = t.rec_base[i] + records[i];
    }
    return t;
}

// ---- the workspaces: WsTake rounds every piece to 256 bytes, so a piece is never merged with another or split ---------------

// the pieces of a vk_clean_device workspace (cl_layout in vkimg.hip); the calls here take the six that cl_index_run fills
struct ClLayout {
    ClFile* files;
    uint64_t *fchunk, *unit_base, *ccount, *cprefix, *sums, *hashes, *obytes, *oprefix;
    ClSample* samples;
    ClRec* recs;
    ClPlan* plans;
    uint32_t *slot_of, *table;
    size_t total;
    uint64_t nchunks, nrec, nslots;
};

// The record index's six pieces for nsamples one-file samples.  `sums` is the scratch of every scan the call makes
// (cl_scan): always the chunks' newline counts, and `also_scanned` items where the call scans something else as well (the
// screen and the depth filter their records' kept bytes, the emit path its items' bytes; the spectrum and QC nothing).
inline void text_index_take(WsTake& take, ClLayout& c, const uint64_t* lengths, const uint64_t* records, uint32_t nsamples,
                            uint64_t also_scanned) {
    for (uint32_t i = 0; i < nsamples; ++i) {
        c.nchunks += (lengths[i] + kClChunk - 1) / kClChunk;
        c.nrec += records[i];
    }
    const uint64_t nb = (std::max(c.nchunks, also_scanned) + kClScanBlock - 1) / kClScanBlock;
    take(c.files, nsamples);
    take(c.fchunk, nsamples);
    take(c.ccount, c.nchunks);
    take(c.cprefix, c.nchunks + 1);
    take(c.sums, nb + 1);
    take(c.recs, c.nrec);
}

// (FaStatePieces, fa_state_take -- the FASTA plan's descriptors and the header state of a batch of FASTA texts, the units
// counted at their smallest size: vk_faplan.h)

// the samples' counting tables as the table kernels read them
struct SpTablePieces {
    uint64_t *block_base, *slot_base, *nslots;
};

inline void sp_tables_take(WsTake& take, SpTablePieces& t, uint32_t nsamples) {
    take(t.block_base, nsamples + 1ull);
    take(t.slot_base, nsamples);
    take(t.nslots, nsamples);
}

// vk_ladder_emit_device: the record index, then the steps' tables and the items' bytes (an item: a step and a record of
// its sample; a step whose sample is out of range has none)
struct EmLayout {
    ClLayout c;
    EmSample* samples;
    EmStep* steps;
    uint64_t *step_base, *sizes, *obytes, *oprefix;
    uint32_t* status;
    size_t total;
    uint64_t nitems;
};

inline EmLayout em_layout(void* d_ws, const uint64_t* records, uint32_t nsamples, const uint64_t* lengths,
                          const uint32_t* step_sample, uint32_t nsteps) {
    EmLayout L{};
    for (uint32_t j = 0; j < nsteps; ++j) L.nitems += step_sample[j] < nsamples ? records[step_sample[j]] : 0;
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    text_index_take(take, L.c, lengths, records, nsamples, L.nitems);
    take(L.samples, nsamples);
    take(L.status, nsamples);
    take(L.steps, nsteps);
    take(L.step_base, nsteps + 1ull);
    take(L.sizes, nsteps);
    take(L.obytes, L.nitems);
    take(L.oprefix, L.nitems + 1);
    L.total = take.at;
    return L;
}

// vk_screen_build_device: one text's header state, then what the build leaves
struct ScBuildLayout {
    FaStatePieces f;
    uint32_t* status;
    ScBuildOut* out;
    size_t total;
};

inline ScBuildLayout sc_build_layout(void* d_ws, uint64_t length) {
    ScBuildLayout L{};
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    fa_state_take(take, L.f, &length, 1);
    take(L.out, 1);
    take(L.status, 1);
    L.total = take.at;
    return L;
}

// vk_screen_device: the record index, then the samples' tables and the records' kept bytes
struct ScLayout {
    ClLayout c;
    EmSample* samples;
    uint64_t *rec_base, *out_offs, *obytes, *oprefix;
    size_t total;
};

inline ScLayout sc_layout(void* d_ws, const uint64_t* records, uint32_t nsamples, const uint64_t* lengths) {
    ScLayout L{};
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    text_index_take(take, L.c, lengths, records, nsamples, text_records(records, nsamples));
    take(L.samples, nsamples);
    take(L.rec_base, nsamples + 1ull);
    take(L.out_offs, nsamples);
    take(L.obytes, L.c.nrec);
    take(L.oprefix, L.c.nrec + 1);
    L.total = take.at;
    return L;
}

// vk_spectrum_device: the record index, then the samples' tables
struct SpLayout {
    ClLayout c;
    EmSample* samples;
    uint64_t* rec_base;
    SpTablePieces t;
    size_t total;
};

inline SpLayout sp_layout(void* d_ws, const uint64_t* records, uint32_t nsamples, const uint64_t* lengths) {
    SpLayout L{};
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    text_index_take(take, L.c, lengths, records, nsamples, 0);
    take(L.samples, nsamples);
    take(L.rec_base, nsamples + 1ull);
    sp_tables_take(take, L.t, nsamples);
    L.total = take.at;
    return L;
}

// vk_spectrum_fasta_device: the texts' header state, then the samples' tables
struct FsLayout {
    FaStatePieces f;
    SpTablePieces t;
    size_t total;
};

inline FsLayout fs_layout(void* d_ws, const uint64_t* lengths, uint32_t nsamples) {
    FsLayout L{};
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    fa_state_take(take, L.f, lengths, nsamples);
    sp_tables_take(take, L.t, nsamples);
    L.total = take.at;
    return L;
}

// vk_depth_device: the screen's, then the samples' tables and bands
struct DpLayout {
    ScLayout s;
    uint64_t *slot_base, *nslots;
    uint32_t *lo, *hi;
    size_t total;
};

inline DpLayout dp_layout(void* d_ws, const uint64_t* records, uint32_t nsamples, const uint64_t* lengths) {
    DpLayout L{};
    L.s = sc_layout(d_ws, records, nsamples, lengths);
    WsTake take{static_cast<uint8_t*>(d_ws), L.s.total};
    take(L.slot_base, nsamples);
    take(L.nslots, nsamples);
    take(L.lo, nsamples);
    take(L.hi, nsamples);
    L.total = take.at;
    return L;
}

// vk_qc_device: the record index, then the streams' tables (QcStream is EmSample: vk_qc.h)
struct QcLayout {
    ClLayout c;
    EmSample* streams;
    uint64_t* block_base;
    uint32_t* bad;
    size_t total;
};

inline QcLayout qc_layout(void* d_ws, const uint64_t* records, const uint64_t* lengths, uint32_t nstreams) {
    QcLayout L{};
    WsTake take{static_cast<uint8_t*>(d_ws), 0};
    text_index_take(take, L.c, lengths, records, nstreams, 0);
    take(L.streams, nstreams);
    take(L.block_base, nstreams + 1ull);
    take(L.bad, nstreams);
    L.total = take.at;
    return L;
}

}  // namespace

#endif  // VK_TEXTPLAN_H
