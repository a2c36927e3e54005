// vk_spectrum.h -- `image / query --kmer-spectrum`: the k-mer spectrum of cleaned reads in HBM, a counting table per sample
// and its histogram.  Part of the one translation unit vkimg.hip (device code for gfx950; see the notes there).
//
// The rule ("`--kmer-spectrum`: the rule"; tests/spectrum_ref.py is the same rule in Python, twice): a
// read's windows are the screen's (vk_screen.h: a base is ACGT of either case, every window of K = 16..31 unbroken bases
// of the sequence line gives the key sc_key); a key is TAKEN when (sc_mix(key) >> 32) % every == 0, and every occurrence
// of a taken key counts.  A sample's row: reads, bases, windows, taken windows, distinct taken keys, and hist[c - 1] = the
// distinct taken keys of multiplicity c (hist[255]: 256 and more).
//
// The tables: per sample nslots (a power of two) u64 keys, the empty slot all ones, and as many u32 counts, at slot_base
// in two caller-allocated buffers.  A key's slot starts at the LOW bits of the mix that selects by its HIGH bits, linear
// probing, insertion by 64-bit compare-and-swap (sc_insert's loop, returning the slot), then one no-return 32-bit add.
//
// Launch sequence of vk_spectrum_device (after the read index, vk_cl_nl_* / vk_cl_scan_*, as the screen uses them):
//   vk_em_status_kernel   per sample: framing (vk_emit.h, unchanged)
//   vk_sp_init_kernel     workgroups over a sample's slots: keys all ones, counts zero
//   vk_sp_count_kernel    wave per record: the screen's LDS tile, a lane per window; equal keys of one wave instruction
//                         are merged before they leave the wave (SpParams::merge), then insert-or-find and the add; the
//                         wave's reads, bases, windows and taken windows flushed when the sample changes
//   vk_sp_hist_kernel     workgroups over a sample's counts: a 256-bin histogram in LDS, flushed with u64 atomics
//   vk_sp_finish_kernel   per sample: a sample with a status gets an all-zero row
//
// The lane-local code (sp_taken, sp_insert, sp_count, sp_bin) compiles for the host: tests/emul/spectrum_emul.cpp runs
// it, a lane at a time, against tests/spectrum_ref.py.
#ifndef VK_SPECTRUM_H
#define VK_SPECTRUM_H

#include <cstdint>

#include "vk_screen.h"

namespace {

constexpr uint32_t kSpNstat = 261;                   // VK_SPEC_NSTAT: reads, bases, windows, taken windows, distinct, hist[256]
constexpr uint32_t kSpHistAt = 5, kSpBins = 256;
constexpr uint32_t kSpTableFull = 32u;               // VK_SPEC_TABLE_FULL (vkimg.h)
constexpr uint64_t kSpNoSlot = ~0ull;
constexpr uint32_t kSpSlotsPerBlock = 16384;         // slots per workgroup of the init and histogram kernels: 64 per lane
constexpr uint32_t kSpHashSlots = 128;               // entries of a wavefront's merge table (SpParams::merge == 2)
constexpr uint32_t kSpMergeDefault = 2;              // SpParams::merge when VKIMG_SPECTRUM_MERGE does not say (what each costs and pays)

// Is the key with this mix taken?  (the HIGH half of the mix selects, the low bits place: sp_insert)
__device__ inline bool sp_taken(uint64_t mix, uint32_t every) { return every == 1u || static_cast<uint32_t>(mix >> 32) % every == 0u; }

// key into the table (nslots a power of two): the slot that holds it -- found or won -- or kSpNoSlot when no slot is
// left.  At most nslots probes, whatever the table holds.
__device__ inline uint64_t sp_insert(uint64_t* keys, uint64_t nslots, uint64_t key, uint64_t mix) {
    uint64_t h = mix & (nslots - 1);
    for (uint64_t n = 0; n < nslots; ++n) {
        unsigned long long* slot = reinterpret_cast<unsigned long long*>(keys + h);
        unsigned long long v = *slot;   // (a slot that holds a key keeps it: a re-hit costs this load alone)
        if (v == kScEmpty) v = atomicCAS(slot, static_cast<unsigned long long>(kScEmpty), static_cast<unsigned long long>(key));
        if (v == kScEmpty || v == key) return h;
        h = (h + 1) & (nslots - 1);
    }
    return kSpNoSlot;
}

#ifndef VK_SPECTRUM_LANE_ONLY
__device__ inline void sp_add(uint32_t* p, uint32_t n) {   // (the result is not used: a no-return atomic)
    (void)__hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

// n occurrences of key: false when the table has no slot for it.
__device__ inline bool sp_count(uint64_t* keys, uint32_t* counts, uint64_t nslots, uint64_t key, uint64_t mix, uint32_t n) {
    const uint64_t slot = sp_insert(keys, nslots, key, mix);
    if (slot == kSpNoSlot) return false;
    sp_add(counts + slot, n);
    return true;
}

// The histogram's bin of a slot's count: kSpBins for a free slot (a held slot counts at least 1).
__device__ inline uint32_t sp_bin(uint32_t count) { return count == 0 ? kSpBins : (count < kSpBins ? count : kSpBins) - 1u; }

#ifndef VK_SPECTRUM_LANE_ONLY

struct SpParams {
    uint64_t* keys;
    uint32_t* counts;
    const uint64_t* slot_base;   // [nsamples] first slot of a sample in keys and counts
    const uint64_t* nslots;      // [nsamples]
    uint32_t K, every, tile;
    uint32_t merge;              // 0: a lane per window adds 1; 1: runs of equal keys in neighbouring lanes add once; 2: and
                                 // equal keys anywhere in the wave instruction, through a table in LDS
};

// the workgroup's sample and its first slot there (block_base: the samples' first workgroups, ascending)
__device__ inline uint32_t sp_locate(const uint64_t* block_base, uint32_t nsamples, uint64_t* first) {
    const uint32_t si = cl_find_u64(block_base, nsamples, blockIdx.x);
    *first = (blockIdx.x - block_base[si]) * kSpSlotsPerBlock;
    return si;
}

__global__ void __launch_bounds__(kClThreads) vk_sp_init_kernel(const uint64_t* block_base, uint32_t nsamples,
                                                               const uint64_t* slot_base, const uint64_t* nslots, uint64_t* keys,
                                                               uint32_t* counts) {
    uint64_t first;
    const uint32_t si = sp_locate(block_base, nsamples, &first);
    const uint64_t n = nslots[si], base = slot_base[si];
    for (uint64_t i = first + threadIdx.x; i < first + kSpSlotsPerBlock && i < n; i += kClThreads) {
        keys[base + i] = kScEmpty;
        counts[base + i] = 0;
    }
}

__global__ void __launch_bounds__(kClThreads) vk_sp_count_kernel(const uint8_t* text, const uint64_t* rec_base, uint32_t nsamples,
                                                                uint64_t nrec, const ClRec* recs, uint32_t* status, SpParams P,
                                                                unsigned long long* rows) {
    __shared__ uint32_t s_codes[kClThreads / 64][kScCodeWords];
    __shared__ uint32_t s_masks[kClThreads / 64][kScMaskWords];
    __shared__ uint32_t s_hash[kClThreads / 64][kSpHashSlots];
    __shared__ uint32_t s_cnt[kClThreads / 64][64];
    const uint32_t wave = sc_uniform(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* codes = s_codes[wave];
    uint32_t* masks = s_masks[wave];
    uint16_t* codes16 = reinterpret_cast<uint16_t*>(codes);
    uint8_t* masks8 = reinterpret_cast<uint8_t*>(masks);
    uint32_t* hash = s_hash[wave];
    uint32_t* cnts = s_cnt[wave];
    const uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kScRecsPerBlock;
    // the wave's sums for the sample of its last record: flushed when the sample changes and at the end
    uint32_t cur = ~0u;
    unsigned long long n_reads = 0, n_bases = 0, n_win = 0, n_taken = 0;
    for (uint32_t j = wave; j < kScRecsPerBlock; j += kClThreads / 64) {
        const uint64_t ri = r0 + j;
        if (ri >= nrec) break;
        const uint32_t si = cl_find_u64(rec_base, nsamples, ri);
        if (sc_uniform(status[si]) != 0) continue;   // (bad framing, or a table that another record found full)
        if (si != cur) {
            if (lane == 0 && cur != ~0u) {
                atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 0, n_reads);
                atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 1, n_bases);
                atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 2, n_win);
                atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 3, n_taken);
            }
            cur = si;
            n_reads = n_bases = n_win = n_taken = 0;
        }
        uint64_t* keys = P.keys + P.slot_base[si];
        uint32_t* counts = P.counts + P.slot_base[si];
        const uint64_t nslots = P.nslots[si];
        const ClRec r = recs[ri];
        const uint8_t* seq = text + r.he + 1;
        uint32_t L = static_cast<uint32_t>(r.se - r.he - 1);
        if (L && seq[L - 1] == '\r') --L;
        L = sc_uniform(L);   // (a scalar: the tile loop is the wave's)
        uint32_t wins = 0, taken_wins = 0, t0 = 0, nb, nw;
        bool full = false;
        while (sc_tile(t0, L, P.tile, P.K, &nb, &nw)) {
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
                bool valid = false;
                uint64_t key = 0, mix = 0;
                if (p < nw) {
                    uint64_t fw;
                    valid = sc_window(codes, masks, p, P.K, &fw);
                    key = sc_key(fw, P.K);
                    mix = sc_mix(key);
                }
                const bool taken = valid && sp_taken(mix, P.every);
                const uint64_t T = __ballot(taken);
                // (the sums are the wave's: kept in scalar registers, so that the loops around them stay the wave's own)
                wins = sc_uniform(wins + static_cast<uint32_t>(__popcll(__ballot(valid))));
                taken_wins = sc_uniform(taken_wins + static_cast<uint32_t>(__popcll(T)));
                bool active = taken;
                uint32_t n = 1;
                if (P.merge >= 1u) {
                    // a run of equal keys in neighbouring lanes (a homopolymer: every lane) adds once, from its first lane
                    const uint64_t prev = __shfl_up(static_cast<unsigned long long>(key), 1, 64);
                    const bool same = taken && lane > 0 && ((T >> (lane - 1u)) & 1ull) != 0 && prev == key;
                    active = taken && !same;
                    const uint64_t H = __ballot(active);
                    const uint64_t stop = (H | ~T) & ~((2ull << lane) - 1ull);   // the first lane behind this one that ends its run
                    n = (stop ? static_cast<uint32_t>(__builtin_ctzll(stop)) : 64u) - lane;
                }
                if (P.merge >= 2u) {
                    // equal keys anywhere in the wave (a tandem repeat: a few keys over and over): a lane writes its number
                    // at its key's entry of the table, the number that stays names the entry's winner, and a lane whose key
                    // is the winner's hands its count over.  (Another key at the same entry loses nothing: it adds itself.)
                    const uint32_t e = static_cast<uint32_t>(mix >> 48) & (kSpHashSlots - 1u);
                    if (active) hash[e] = lane;
                    cnts[lane] = n;
                    sc_wave_lds_fence();
                    const uint32_t w = active ? hash[e] : lane;
                    const uint64_t wkey = __shfl(static_cast<unsigned long long>(key), static_cast<int>(w), 64);
                    const bool dup = active && w != lane && wkey == key;
                    if (dup) atomicAdd(cnts + w, n);
                    sc_wave_lds_fence();
                    n = cnts[lane];
                    active = active && !dup;
                    sc_wave_lds_fence();   // (read before the next trip writes)
                }
                if (active && !sp_count(keys, counts, nslots, key, mix, n)) full = true;
            }
            t0 = sc_uniform(t0 + nw);
        }
        if (full) atomicOr(status + si, kSpTableFull);   // (the sample's row is zeroed at the end; its other records stop early)
        ++n_reads;
        n_bases += L;
        n_win += wins;
        n_taken += taken_wins;
    }
    if (lane == 0 && cur != ~0u) {
        atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 0, n_reads);
        atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 1, n_bases);
        atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 2, n_win);
        atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * cur + 3, n_taken);
    }
}

__global__ void __launch_bounds__(kClThreads) vk_sp_hist_kernel(const uint64_t* block_base, uint32_t nsamples,
                                                               const uint64_t* slot_base, const uint64_t* nslots,
                                                               const uint32_t* counts, const uint32_t* status,
                                                               unsigned long long* rows) {
    __shared__ uint32_t s_hist[kSpBins];
    uint64_t first;
    const uint32_t si = sp_locate(block_base, nsamples, &first);
    if (status[si] != 0) return;   // (uniform: the whole workgroup)
    s_hist[threadIdx.x] = 0;
    static_assert(kSpBins == kClThreads, "a bin per thread");
    __syncthreads();
    const uint64_t n = nslots[si];
    const uint32_t* c = counts + slot_base[si];
    // singletons -- most of a shallow skim's keys -- are summed in a register, not at one LDS address
    uint32_t ones = 0, held = 0;
    for (uint64_t i = first + threadIdx.x; i < first + kSpSlotsPerBlock && i < n; i += kClThreads) {
        const uint32_t b = sp_bin(c[i]);
        if (b == 0) ++ones;
        else if (b < kSpBins) atomicAdd(&s_hist[b], 1u);
        held += b < kSpBins ? 1u : 0u;
    }
    for (uint32_t d = 32; d; d >>= 1) {
        ones += __shfl_down(ones, d, 64);
        held += __shfl_down(held, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (ones) atomicAdd(&s_hist[0], ones);
        if (held) atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * si + 4, static_cast<unsigned long long>(held));
    }
    __syncthreads();
    const uint32_t v = s_hist[threadIdx.x];
    if (v) atomicAdd(rows + static_cast<uint64_t>(kSpNstat) * si + kSpHistAt + threadIdx.x, static_cast<unsigned long long>(v));
}

__global__ void __launch_bounds__(kClThreads) vk_sp_finish_kernel(const uint32_t* status, unsigned long long* rows) {
    if (status[blockIdx.x] == 0) return;
    for (uint32_t i = threadIdx.x; i < kSpNstat; i += kClThreads) rows[static_cast<uint64_t>(kSpNstat) * blockIdx.x + i] = 0;
}

#endif  // VK_SPECTRUM_LANE_ONLY

}  // namespace

#endif  // VK_SPECTRUM_H
