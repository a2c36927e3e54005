// vk_depth.h -- `image / query --kmer-spectrum --depth-filter`: cleaned reads kept by the depth of their own k-mers in
// their sample's spectrum table, while that lies in HBM.  Part of the one translation unit vkimg.hip (device code for
// gfx950; see the notes there).
//
// The rule ("`--depth-filter`: the rule"; tests/depth_ref.py is the same rule in Python, twice): a read's
// windows and keys are the spectrum's (vk_screen.h, vk_spectrum.h); the depth c(w) of a TAKEN window is the count in the
// slot of the sample's table that holds its key, 0 when none does; a record's depth m is the lower median of its taken
// windows' depths -- the element at index (n - 1) / 2 of the sorted c(w) -- and 0 for a record without one; the record is
// kept when lo <= m <= hi, copied whole, byte for byte, in input order.  A sample's row: records in, records kept,
// sequence bases in, sequence bases kept, records without a taken window, and hist[min(m, 255)] over ALL records in.
//
// The decision does not go through the histogram, which saturates: m >= lo iff #{c < lo} <= (n - 1) / 2 and m <= hi iff
// #{c <= hi} > (n - 1) / 2, two counts the wave keeps beside n.  It is exact for any u32 bounds.
//
// Launch sequence of vk_depth_device (after the read index, vk_cl_nl_* / vk_cl_scan_*, as the screen uses them):
//   vk_em_status_kernel   per sample: framing (vk_emit.h, unchanged)
//   vk_dp_status_kernel   per sample: the spectrum's status joins the framing's (a table that filled is no table)
//   vk_dp_match_kernel    wave per record: the screen's LDS tile, a lane per window, one read-only probe and one count
//                         loaded per taken window, a 256-bin histogram of the wave in LDS; the bytes the record keeps
//   vk_cl_scan_*          exclusive scan of the records' kept bytes
//   vk_sc_write_kernel    wave per record: the record's bytes (vk_screen.h, unchanged)
//   vk_sc_pad_kernel      per sample: its length, zeros up to the 16-byte rounded end (vk_screen.h, unchanged)
//
// The lane-local code (sp_find, dp_bin, dp_kept, dp_decide, dp_lane_bin, dp_median_bin) compiles for the host:
// tests/emul/depth_emul.cpp runs it, a lane at a time, against tests/depth_ref.py.
#ifndef VK_DEPTH_H
#define VK_DEPTH_H

#include <cstdint>

#include "vk_spectrum.h"

namespace {

constexpr uint32_t kDpNstat = 261;                   // VK_DEPTH_NSTAT: in, kept, bases in, bases kept, without windows, hist[256]
constexpr uint32_t kDpHistAt = 5, kDpBins = 256;     // VK_DEPTH_HIST
constexpr uint32_t kDpMergeDefault = 0;              // DpParams::merge when VKIMG_DEPTH_MERGE does not say: plain (no difference was measured)

// The slot of the table (nslots a power of two) that holds key, kSpNoSlot when none does: sp_insert's walk without its
// compare-and-swap.  It stops at a free slot or after nslots probes, whatever the table holds; it never writes.
__device__ inline uint64_t sp_find(const uint64_t* keys, uint64_t nslots, uint64_t key, uint64_t mix) {
    uint64_t h = mix & (nslots - 1);
    for (uint64_t n = 0; n < nslots; ++n) {
        const uint64_t v = keys[h];
        if (v == key) return h;
        if (v == kScEmpty) return kSpNoSlot;
        h = (h + 1) & (nslots - 1);
    }
    return kSpNoSlot;
}

// The histogram's bin of a depth: 255 holds that and more.
__device__ inline uint32_t dp_bin(uint32_t c) { return c < kDpBins - 1u ? c : kDpBins - 1u; }

// A record of n >= 1 taken windows, below_lo of them with c < lo and at_most_hi with c <= hi: is lo <= median <= hi?
__device__ inline bool dp_kept(uint32_t n, uint32_t below_lo, uint32_t at_most_hi) {
    const uint32_t r = (n - 1u) / 2u;
    return below_lo <= r && at_most_hi > r;
}

// The same for any n: a record without a taken window has depth 0, as if its one window were absent from the table.
__device__ inline bool dp_decide(uint32_t n, uint32_t below_lo, uint32_t at_most_hi, uint32_t lo) {
    return n ? dp_kept(n, below_lo, at_most_hi) : dp_kept(1u, lo > 0u ? 1u : 0u, 1u);
}

// A lane's part of the median: h4 its four consecutive bins, excl the sum of every bin before them.  The one of its bins
// (0..3) that holds rank, 4 when none of them does.
__device__ inline uint32_t dp_lane_bin(const uint32_t* h4, uint32_t excl, uint32_t rank) {
    uint32_t at = excl;
    for (uint32_t i = 0; i < 4; ++i) {
        if (rank >= at && rank - at < h4[i]) return i;
        at += h4[i];
    }
    return 4u;
}

// The bin that holds the lower median of a record's histogram of n entries (hist[dp_bin(c)] over its taken windows):
// min(m, 255).  0 for n == 0.  The lanes' walk of the kernel, one lane after the other.
__device__ inline uint32_t dp_median_bin(const uint32_t* hist, uint32_t n) {
    if (n == 0) return 0u;
    uint32_t excl = 0;
    for (uint32_t lane = 0; lane < kDpBins / 4u; ++lane) {
        const uint32_t b = dp_lane_bin(hist + 4u * lane, excl, (n - 1u) / 2u);
        if (b < 4u) return 4u * lane + b;
        excl += hist[4u * lane] + hist[4u * lane + 1] + hist[4u * lane + 2] + hist[4u * lane + 3];
    }
    return kDpBins - 1u;   // (not reached when the bins sum to n)
}

#ifndef VK_SPECTRUM_LANE_ONLY

struct DpParams {
    const uint64_t* keys;
    const uint32_t* counts;
    const uint64_t* slot_base;   // [nsamples] first slot of a sample in keys and counts
    const uint64_t* nslots;      // [nsamples]
    const uint32_t* lo;          // [nsamples] the band, both ends included
    const uint32_t* hi;
    uint32_t K, every, tile;
    uint32_t merge;              // 0: every taken lane adds 1 at its bin; 1: a wave instruction whose taken lanes all hold
                                 // one bin (a homopolymer, a shallow skim's singletons) adds once, from its first lane
};

__global__ void __launch_bounds__(kClThreads) vk_dp_status_kernel(const uint32_t* table_status, uint32_t nsamples, uint32_t* status) {
    const uint32_t si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si < nsamples) status[si] |= table_status[si];
}

__device__ inline void dp_flush(unsigned long long* rows, uint32_t si, const unsigned long long* sums) {
    for (uint32_t i = 0; i < kDpHistAt; ++i)
        if (sums[i]) atomicAdd(rows + static_cast<uint64_t>(kDpNstat) * si + i, sums[i]);
}

__global__ void __launch_bounds__(kClThreads) vk_dp_match_kernel(const uint8_t* text, const EmSample* samples,
                                                                const uint64_t* rec_base, uint32_t nsamples, uint64_t nrec,
                                                                const ClRec* recs, const uint32_t* status, DpParams P,
                                                                uint64_t* out_bytes, unsigned long long* rows) {
    __shared__ uint32_t s_codes[kClThreads / 64][kScCodeWords];
    __shared__ uint32_t s_masks[kClThreads / 64][kScMaskWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[kClThreads / 64][kDpBins];
    static_assert(kDpBins == 4 * 64, "four bins per lane");
    const uint32_t wave = sc_uniform(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* codes = s_codes[wave];
    uint32_t* masks = s_masks[wave];
    uint16_t* codes16 = reinterpret_cast<uint16_t*>(codes);
    uint8_t* masks8 = reinterpret_cast<uint8_t*>(masks);
    uint32_t* hist = s_hist[wave];
    uint4* mine = reinterpret_cast<uint4*>(hist) + lane;   // the lane's four consecutive bins
    *mine = make_uint4(0, 0, 0, 0);
    const uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kScRecsPerBlock;
    // the wave's sums for the sample of its last record: flushed when the sample changes and at the end
    uint32_t cur = ~0u;
    unsigned long long sums[kDpHistAt] = {};   // records in, kept, bases in, bases kept, records without a taken window
    for (uint32_t j = wave; j < kScRecsPerBlock; j += kClThreads / 64) {
        const uint64_t ri = r0 + j;
        if (ri >= nrec) break;
        const uint32_t si = cl_find_u64(rec_base, nsamples, ri);
        if (sc_uniform(status[si]) != 0) {   // (bad framing, or no table)
            if (lane == 0) out_bytes[ri] = 0;
            continue;
        }
        if (si != cur) {
            if (lane == 0 && cur != ~0u) dp_flush(rows, cur, sums);
            cur = si;
            for (uint32_t i = 0; i < kDpHistAt; ++i) sums[i] = 0;
        }
        const uint64_t* keys = P.keys + P.slot_base[si];
        const uint32_t* counts = P.counts + P.slot_base[si];
        const uint64_t nslots = P.nslots[si];
        const uint32_t lo = sc_uniform(P.lo[si]), hi = sc_uniform(P.hi[si]);
        const EmSample s = samples[si];
        const ClRec r = recs[ri];
        const uint8_t* seq = text + r.he + 1;
        uint32_t L = static_cast<uint32_t>(r.se - r.he - 1);
        if (L && seq[L - 1] == '\r') --L;
        L = sc_uniform(L);   // (a scalar: the tile loop is the wave's)
        uint32_t n = 0, below = 0, atmost = 0, t0 = 0, nb, nw;
        while (sc_tile(t0, L, P.tile, P.K, &nb, &nw)) {   // (no early exit: the histogram needs the whole read)
            sc_wave_lds_fence();   // (the windows of the tile before are read)
            for (uint32_t c = lane; c < (nb + 7u) / 8u; c += 64) {
                uint16_t code;
                uint8_t mask;
                sc_pack8(seq + t0 + 8u * c, min(8u, nb - 8u * c), &code, &mask);
                codes16[c ^ 1u] = code;
                masks8[c ^ 3u] = mask;
            }
            sc_wave_lds_fence();
            for (uint32_t p0 = 0; p0 < nw; p0 = sc_uniform(p0 + 64u)) {
                const uint32_t p = p0 + lane;
                bool taken = false;
                uint32_t c = 0;
                if (p < nw) {
                    uint64_t fw;
                    if (sc_window(codes, masks, p, P.K, &fw)) {
                        const uint64_t key = sc_key(fw, P.K), mix = sc_mix(key);
                        taken = sp_taken(mix, P.every);
                        if (taken) {
                            const uint64_t slot = sp_find(keys, nslots, key, mix);
                            c = slot == kSpNoSlot ? 0u : counts[slot];
                        }
                    }
                }
                const uint64_t T = __ballot(taken);
                // (the sums are the wave's: kept in scalar registers, so that the loops around them stay the wave's own)
                n = sc_uniform(n + static_cast<uint32_t>(__popcll(T)));
                below = sc_uniform(below + static_cast<uint32_t>(__popcll(__ballot(taken && c < lo))));
                atmost = sc_uniform(atmost + static_cast<uint32_t>(__popcll(__ballot(taken && c <= hi))));
                const uint32_t bin = dp_bin(c);
                bool add = taken;
                uint32_t amount = 1;
                if (P.merge >= 1u && T) {
                    const uint32_t first = static_cast<uint32_t>(__builtin_ctzll(T));
                    const uint32_t fbin = static_cast<uint32_t>(__shfl(static_cast<int>(bin), static_cast<int>(first), 64));
                    if (__ballot(taken && bin == fbin) == T) {   // one bin: one add
                        add = lane == first;
                        amount = static_cast<uint32_t>(__popcll(T));
                    }
                }
                if (add) atomicAdd(hist + bin, amount);
            }
            t0 = sc_uniform(t0 + nw);
        }
        // the median's bin: a lane sums its four bins, a scan over the wave finds the lane that holds rank (n - 1) / 2
        sc_wave_lds_fence();
        const uint4 h = *mine;
        *mine = make_uint4(0, 0, 0, 0);   // (clean for the next record)
        const uint32_t h4[4] = {h.x, h.y, h.z, h.w};
        const uint32_t own = h.x + h.y + h.z + h.w;
        uint32_t incl = own;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        uint32_t mbin = 0;
        if (n) {
            const uint32_t b = dp_lane_bin(h4, incl - own, (n - 1u) / 2u);
            const uint64_t holds = __ballot(b < 4u);   // (one lane, as the bins sum to n)
            const uint32_t src = holds ? static_cast<uint32_t>(__builtin_ctzll(holds)) : 0u;
            mbin = static_cast<uint32_t>(__shfl(static_cast<int>(4u * lane + (b & 3u)), static_cast<int>(src), 64));
        }
        const bool kept = dp_decide(n, below, atmost, lo);
        ++sums[0];
        sums[2] += L;
        if (kept) {
            ++sums[1];
            sums[3] += L;
        }
        if (n == 0) ++sums[4];
        if (lane == 0) {
            out_bytes[ri] = kept ? sc_rec_end(r, s) - r.h : 0;
            atomicAdd(rows + static_cast<uint64_t>(kDpNstat) * si + kDpHistAt + mbin, 1ull);
        }
    }
    if (lane == 0 && cur != ~0u) dp_flush(rows, cur, sums);
}

#endif  // VK_SPECTRUM_LANE_ONLY

}  // namespace

#endif  // VK_DEPTH_H
