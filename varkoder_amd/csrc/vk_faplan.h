// vk_faplan.h -- the host's side of the calls that count from FASTA text in HBM: vk_count_fasta_device (vk_fasta.h),
// vk_count_fasta_sampled_device (vk_fasta_ladder.h), vk_fasta_records_count_device, vk_fasta_records_device and
// vk_count_fasta_records_device (vk_fasta_records.h) and vk_count_fasta_windows_device (vk_fasta_windows.h); the plan and
// the header state's pieces serve vk_screen_build_device and vk_spectrum_fasta_device as well (vk_textplan.h).  What a call
// carries, the rules its arguments must keep, how a batch is cut into units and workgroups, the pair table of the sampled
// call and the pieces of the workspaces.  They run on caller input and are plain functions of a few integer arrays: no HIP
// here, so that a host compiler and a CPU test reach them (tests/emul/faplan_emul.cpp).
//
// The constants and the plain structs stay where the kernels use them: vkimg.hip includes this header behind the device
// headers; a host compiler gets their plain part through it (VK_FASTA_LANE_ONLY).
//
// Every rule here answers VK_EINVAL, so among the rules of one call the order shows only against what is NOT a refusal.
// Known warts, kept (callers can observe them, so they are written down and tested, tests/faplan_emul_lib.py, not fixed):
//   * nsamples == 0.  vk_count_fasta_device, vk_count_fasta_sampled_device, vk_fasta_records_count_device and
//     vk_fasta_records_device answer VK_OK once their rules hold, before they look at d_fasta and without writing anything.
//     vk_count_fasta_records_device and vk_count_fasta_windows_device look at d_fasta only when nsamples != 0; with no
//     sample they reset d_hist and then answer VK_OK.
//   * Those two check the offsets' alignment themselves (fa_offsets_ok), because they reset d_hist BEFORE the plan is made:
//     a misaligned offset is refused with d_hist untouched, a batch that only the plan refuses (2^30 units in a sample,
//     2^31 workgroups) with d_hist already zero.  The other four calls write nothing before their last refusal.
#ifndef VK_FAPLAN_H
#define VK_FAPLAN_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "vkimg.h"
#ifndef VK_FASTA_WINDOWS_H
#ifndef __HIPCC__
#define __device__
#define __host__
#endif
#define VK_FASTA_LANE_ONLY
#include "vk_fasta_windows.h"
#endif
#include "vk_ws.h"

namespace {

// What a FASTA call passes around, whichever it is; a call leaves what it does not have at null or 0.  The arrays are the
// caller's, on the host.
struct FaCall {
    const uint64_t *offsets, *lengths;   // one entry per sample
    uint32_t nsamples;
    int k;
    const uint64_t* rec_first;           // [nsamples + 1] the ordinal of a sample's first record
    uint32_t nslots;                     // rows of the per-record count
    const uint32_t* pair_sample;         // the sampled call's pairs, npairs entries each
    const uint64_t *seeds, *thresholds, *shifts;
    uint32_t npairs, frag_len;
    uint32_t win_len, win_step, nrows, tile_rows;   // the windows
};

// ---- the unit and the plan ---------------------------------------------------------------------------------------------

// VKIMG_FASTA_UNIT_BYTES as a context keeps it: 0 (not set) stays 0, else whole lanes, one at least, a full unit at most.
inline uint32_t fa_unit_clamp(uint32_t env) {
    if (env == 0) return 0;
    env = env / kFaLaneBytes * kFaLaneBytes;
    if (env < kFaLaneBytes) env = kFaLaneBytes;
    return env > kFaUnitBytes ? kFaUnitBytes : env;
}

inline bool fa_offset_ok(uint64_t offset) { return (offset & 15u) == 0; }   // (a lane loads 16 bytes at a time)

inline bool fa_offsets_ok(const uint64_t* offsets, uint32_t nsamples) {
    for (uint32_t i = 0; i < nsamples; ++i)
        if (!fa_offset_ok(offsets[i])) return false;
    return true;
}

// How a batch of FASTA samples is cut: meta = offsets | lengths | first workgroup | first unit of every sample.
struct FaPlan {
    std::vector<uint64_t> meta;
    uint32_t nsamples = 0, unit = 0, span = 0;
    uint64_t nwg = 0, nunits = 0;
    const uint64_t* wg_first() const { return meta.data() + 2ull * nsamples; }
    FaMeta on_device(const uint64_t* d_meta) const {
        return FaMeta{d_meta, d_meta + nsamples, d_meta + 2ull * nsamples, d_meta + 3ull * nsamples + 1, nsamples, unit, span};
    }
    uint64_t lane_words() const { return nunits * (unit / kFaLaneBytes) + 1; }   // the index: a word per lane of text, 1/16 of it
};

// unit_override: the context's fa_unit_clamp(VKIMG_FASTA_UNIT_BYTES); 0: full units, kFaSpanUnits of them per workgroup.
inline int fa_plan(uint32_t unit_override, const uint64_t* offsets, const uint64_t* lengths, uint32_t nsamples, FaPlan* pl) {
    pl->nsamples = nsamples;
    pl->unit = unit_override ? unit_override : kFaUnitBytes;
    pl->span = unit_override ? 1u : kFaSpanUnits;
    pl->meta.assign(4ull * nsamples + 2, 0);
    uint64_t* wg_first = pl->meta.data() + 2ull * nsamples;
    uint64_t* unit_first = wg_first + nsamples + 1;
    for (uint32_t i = 0; i < nsamples; ++i) {
        if (!fa_offset_ok(offsets[i])) return VK_EINVAL;
        const uint64_t units = (lengths[i] + pl->unit - 1) / pl->unit;
        if (units >= (1ull << 30)) return VK_EINVAL;   // (a unit's number takes 31 bits of the scan's key)
        pl->meta[i] = offsets[i];
        pl->meta[nsamples + i] = lengths[i];
        wg_first[i + 1] = wg_first[i] + (units + pl->span - 1) / pl->span;
        unit_first[i + 1] = unit_first[i] + units;
    }
    pl->nwg = wg_first[nsamples];
    pl->nunits = unit_first[nsamples];
    return pl->nwg >= (1ull << 31) ? VK_EINVAL : VK_OK;
}

// ---- the argument rules (the context, the null pointers and d_fasta's alignment are the entry points' to check) --------

inline bool fa_k_ok(int k) { return k >= 5 && k <= 9; }

inline bool far_rec_first_ok(const uint64_t* rec_first, uint32_t nsamples) {
    if (rec_first[0] != 0) return false;
    for (uint32_t i = 0; i < nsamples; ++i)
        if (rec_first[i + 1] < rec_first[i]) return false;
    return true;
}

// The windows: *steps = tiles of a window (win_len / win_step).
inline int faw_window_check(const FaCall& c, uint32_t* steps) {
    if (c.win_step < static_cast<uint32_t>(c.k) || c.win_len >= (1u << 31) || c.win_len < c.win_step || c.win_len % c.win_step != 0)
        return VK_EINVAL;
    *steps = c.win_len / c.win_step;
    return *steps > kFaMaxSteps || c.nrows == 0 || (*steps > 1 && c.tile_rows == 0) ? VK_EINVAL : VK_OK;
}

// *sum_wgs = the workgroups of vk_faw_sum_kernel (none when a window is one tile).
inline int faw_sum_check(const FaCall& c, uint32_t steps, uint64_t* sum_wgs) {
    const uint64_t ncode = 1ull << (2 * c.k);
    *sum_wgs = steps > 1 ? static_cast<uint64_t>(c.tile_rows) * (ncode / kFawSumCodes) : 0;
    return *sum_wgs >= (1ull << 31) ? VK_EINVAL : VK_OK;
}

// The calls' rules up to where the entry point looks at d_fasta, each in the order its entry point has always applied them.

inline int count_fasta_check(const FaCall& c) { return fa_k_ok(c.k) ? VK_OK : VK_EINVAL; }

inline int count_fasta_sampled_check(const FaCall& c) {
    if (!fa_k_ok(c.k) || c.frag_len < static_cast<uint32_t>(c.k) || c.frag_len >= (1u << 31)) return VK_EINVAL;
    for (uint32_t i = 0; i < c.npairs; ++i)   // (q + shift stays below 2^64: ordinals are below 2^63)
        if (c.pair_sample[i] >= c.nsamples || c.thresholds[i] > (1ull << 32) || c.shifts[i] >= (1ull << 63)) return VK_EINVAL;
    return VK_OK;
}

inline int fasta_records_count_check(const FaCall&) { return VK_OK; }   // (the plan's rules are all it has)

inline int fasta_records_check(const FaCall& c) { return far_rec_first_ok(c.rec_first, c.nsamples) ? VK_OK : VK_EINVAL; }

inline int count_fasta_records_check(const FaCall& c) {
    if (!fa_k_ok(c.k) || c.nslots == 0 || c.nslots == kFaNoSlot) return VK_EINVAL;
    return far_rec_first_ok(c.rec_first, c.nsamples) ? VK_OK : VK_EINVAL;
}

inline int count_fasta_windows_check(const FaCall& c, uint32_t* steps) {
    if (!fa_k_ok(c.k)) return VK_EINVAL;
    if (int rc = faw_window_check(c, steps)) return rc;
    return far_rec_first_ok(c.rec_first, c.nsamples) ? VK_OK : VK_EINVAL;
}

// ---- the pair table of the sampled call -------------------------------------------------------------------------------------

// words = sample | seed | threshold | shift | first workgroup of every pair: a pair runs its sample's workgroups.
struct FaPairPlan {
    std::vector<uint64_t> words;
    uint32_t npairs = 0;
    uint64_t pair_nwg = 0;
    FaPairs pairs_on_device(const uint64_t* d_pairs, uint32_t frag_len) const {
        return FaPairs{d_pairs, d_pairs + npairs, d_pairs + 2ull * npairs, d_pairs + 3ull * npairs, d_pairs + 4ull * npairs, npairs,
                       frag_len};
    }
};

// c: checked by count_fasta_sampled_check; pl: its samples' plan.
inline int fa_pair_plan(const FaCall& c, const FaPlan& pl, FaPairPlan* pp) {
    const uint32_t npairs = pp->npairs = c.npairs;
    pp->words.assign(5ull * npairs + 1, 0);
    uint64_t* pair_wg = pp->words.data() + 4ull * npairs;
    for (uint32_t i = 0; i < npairs; ++i) {
        pp->words[i] = c.pair_sample[i];
        pp->words[npairs + i] = c.seeds[i];
        pp->words[2ull * npairs + i] = c.thresholds[i];
        pp->words[3ull * npairs + i] = c.shifts[i];
        pair_wg[i + 1] = pair_wg[i] + (pl.wg_first()[c.pair_sample[i] + 1] - pl.wg_first()[c.pair_sample[i]]);
    }
    pp->pair_nwg = pair_wg[npairs];
    return pp->pair_nwg >= (1ull << 31) ? VK_EINVAL : VK_OK;
}

// ---- the workspaces: WsTake rounds every piece to 256 bytes, so a piece is never merged with another or split ---------------

// The plan's descriptors and the header state of a batch of FASTA texts (vk_fasta.h): what vk_count_fasta_device takes.
struct FaStatePieces {
    uint64_t* meta;
    uint32_t *ukey, *carry;
};

// A workspace of the context is carved when the plan is made, for the plan's units ...
inline void fa_state_take(WsTake& take, FaStatePieces& p, uint32_t nsamples, uint64_t nunits) {
    take(p.meta, 4ull * nsamples + 2);
    take(p.ukey, nunits + 1);
    take(p.carry, nunits + 1);
}

// ... a workspace of the caller is sized before a context is there: the units counted at their smallest size, a lane each.
inline void fa_state_take(WsTake& take, FaStatePieces& p, const uint64_t* lengths, uint32_t nsamples) {
    uint64_t nunits = 0;
    for (uint32_t i = 0; i < nsamples; ++i) nunits += (lengths[i] + kFaLaneBytes - 1) / kFaLaneBytes;
    fa_state_take(take, p, nsamples, nunits);
}

// vk_count_fasta_sampled_device: the pair table behind the descriptors, then the units' ordinals and the lanes' index
struct FaSampledPieces {
    FaStatePieces f;
    uint64_t* pairs;
    unsigned long long* unit_ord;
    uint32_t* lane;
};

inline void fa_sampled_take(WsTake& take, FaSampledPieces& p, const FaPlan& pl, uint32_t npairs) {
    take(p.f.meta, pl.meta.size());
    take(p.pairs, 5ull * npairs + 1);
    take(p.f.ukey, pl.nunits + 1);
    take(p.f.carry, pl.nunits + 1);
    take(p.unit_ord, pl.nunits + 1);
    take(p.lane, pl.lane_words());
}

// the three per-record calls and the windows (far_prepare): uhdr the header lines before every unit; status and nrec
// where they are not the caller's
struct FarPieces {
    uint64_t *meta, *rec_first;
    uint32_t *ukey, *carry, *uhdr, *status, *nrec;
};

inline void far_take(WsTake& take, FarPieces& p, const FaPlan& pl) {
    take(p.meta, pl.meta.size());
    take(p.rec_first, pl.nsamples + 1ull);
    take(p.ukey, pl.nunits + 1);
    take(p.carry, pl.nunits + 1);
    take(p.uhdr, pl.nunits + 1);
    take(p.status, pl.nsamples);
    take(p.nrec, pl.nsamples);
}

// vk_count_fasta_windows_device, a workspace of its own beside far_prepare's: total the records of the batch; the tiles'
// rows only where a window is more than one tile
struct FawPieces {
    uint32_t* lane;
    unsigned long long *unit_ord, *bases;
    FawRec* recs;
    uint32_t *used, *tiles;
};

inline void faw_take(WsTake& take, FawPieces& p, const FaPlan& pl, uint64_t total, uint32_t steps, uint32_t tile_rows, int k) {
    take(p.lane, pl.lane_words());
    take(p.unit_ord, pl.nunits + 1);
    take(p.bases, pl.nsamples);
    take(p.recs, total + 1);
    take(p.used, 1);
    take(p.tiles, steps > 1 ? static_cast<size_t>(tile_rows) << (2 * k) : 1);
}

}  // namespace

#endif  // VK_FAPLAN_H
