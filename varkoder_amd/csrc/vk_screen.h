// vk_screen.h -- `image / query --exclude-fasta / --keep-fasta`: a k-mer screen of cleaned reads against a reference
// FASTA, both in HBM.  Part of the one translation unit vkimg.hip (device code for gfx950; see the notes there).
//
// The rule ("--exclude-fasta / --keep-fasta: the rule"; tests/screen_ref.py is the same rule in Python,
// twice): the reference's lines, headers and records are vk_fasta.h's; a base is ACGT of either case, coded 0 1 2 3; every
// window of K (16..31) unbroken bases gives a key, the smaller of the window and its reverse complement as 2K-bit
// integers, first base most significant; the set is the distinct keys.  A read's windows come the same way from its
// sequence line; it matches when at least min_hits window POSITIONS have their key in the set.  A record is kept (or
// dropped) whole, byte for byte.
//
// The set: open addressing over u64 keys, linear probing, the empty slot all ones, insertion by 64-bit compare-and-swap.
// Built from the text as it lies (no compaction: vk_fasta.h's header state tells which bytes are sequence, and a lane
// reads forward across line seams for the K - 1 further bases its open windows need, as the count does):
//   vk_fa_summary_kernel / vk_fa_scan_kernel   the header state that enters every unit (vk_fasta.h, unchanged)
//   vk_sc_build_kernel<false>                  the number of windows (the caller sizes the table from it)
//   vk_sc_build_kernel<true>                   every window's key into the table; the distinct keys are the slots won
//
// Launch sequence of vk_screen_device (after the read index, vk_cl_nl_* / vk_cl_scan_*, as the emit path uses them):
//   vk_em_status_kernel   per sample: framing (vk_emit.h, unchanged)
//   vk_sc_match_kernel    wave per record: the sequence packed to 2 bits a base plus a break mask in LDS, a lane per
//                         window position, the hits summed over the wave; the bytes the record keeps
//   vk_cl_scan_*          exclusive scan of the records' kept bytes
//   vk_sc_write_kernel    wave per record: the record's bytes, lanes on consecutive bytes
//   vk_sc_pad_kernel      per sample: its length, zeros up to the 16-byte rounded end
//
// The lane-local code (sc_revcomp, sc_pack8, sc_window, sc_probe, sc_insert, sc_tile, ScWalk) compiles for the host:
// tests/emul/screen_emul.cpp runs it, a lane at a time, against tests/screen_ref.py.
#ifndef VK_SCREEN_H
#define VK_SCREEN_H

#include <cstdint>

#ifndef VK_SCREEN_LANE_ONLY
#include "vk_emit.h"
#include "vk_fasta.h"
#endif

namespace {

constexpr uint64_t kScEmpty = ~0ull;                 // a free slot: no key of at most 62 bits equals it
constexpr uint32_t kScMinK = 16, kScMaxK = 31;
constexpr uint64_t kScMinSlots = 1024;
constexpr uint32_t kScMaxTile = 4096;                // bases of a wavefront's LDS tile (VKIMG_SCREEN_TILE shrinks it)
constexpr uint32_t kScRecsPerBlock = 64;             // records per workgroup of the match and write kernels (16 per wavefront)
constexpr uint32_t kScCodeWords = kScMaxTile / 16 + 2, kScMaskWords = kScMaxTile / 32 + 1;   // (a window reads 3 and 2 words)

__device__ inline uint32_t sc_code(uint32_t b) {   // A0 C1 G2 T3 in either case; 4: every other byte
    const uint32_t u = b & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// splitmix64's finaliser, a bijection on u64.  It defines the content of a file: the values of `<sample>.sketch.npy`
// (vk_sketch.h, "hash": "splitmix64-finaliser", version 1) are these, so the mix stays as it is.
__device__ inline uint64_t sc_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The reverse complement of a window of K bases held in the low 2K bits of fw (first base most significant): the
// complement of a code is its bitwise NOT, the order of the 2-bit groups is turned round with three swaps and a byte swap.
__device__ inline uint64_t sc_revcomp(uint64_t fw, uint32_t K) {
    uint64_t x = ~fw;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = __builtin_bswap64(x);
    return x >> (64u - 2u * K);
}

__device__ inline uint64_t sc_key(uint64_t fw, uint32_t K) {
    const uint64_t rc = sc_revcomp(fw, K);
    return fw < rc ? fw : rc;
}

// Is key in the table (nslots a power of two)?  At most nslots probes, whatever the table holds.
__device__ inline bool sc_probe(const uint64_t* table, uint64_t nslots, uint64_t key) {
    uint64_t h = sc_mix(key) & (nslots - 1);
    for (uint64_t n = 0; n < nslots; ++n) {
        const uint64_t v = table[h];
        if (v == key) return true;
        if (v == kScEmpty) return false;
        h = (h + 1) & (nslots - 1);
    }
    return false;
}

// key into the table: 1 = this call won a free slot (a new distinct key), 0 = the key was there, 2 = no slot left.
__device__ inline uint32_t sc_insert(uint64_t* table, uint64_t nslots, uint64_t key) {
    uint64_t h = sc_mix(key) & (nslots - 1);
    for (uint64_t n = 0; n < nslots; ++n) {
        unsigned long long* slot = reinterpret_cast<unsigned long long*>(table + h);
        unsigned long long v = *slot;
        if (v == kScEmpty) v = atomicCAS(slot, static_cast<unsigned long long>(kScEmpty), static_cast<unsigned long long>(key));
        if (v == kScEmpty) return 1u;
        if (v == key) return 0u;
        h = (h + 1) & (nslots - 1);
    }
    return 2u;
}

// Eight bases of a tile, p[0 .. n) (n <= 8; the rest counts as breaks): their codes as 16 bits, first base most
// significant, and a break bit per base the same way round.  Chunk j of a tile goes to u16 j ^ 1 of the code words and
// byte j ^ 3 of the mask words, so that base i of the tile lies at bits 31 - 2 (i % 16) .. of code word i / 16 and at bit
// 31 - i % 32 of mask word i / 32 (little-endian words).
__device__ inline void sc_pack8(const uint8_t* p, uint32_t n, uint16_t* code, uint8_t* mask) {
    uint32_t c = 0, m = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t v = i < n ? sc_code(p[i]) : 4u;
        c = (c << 2) | (v & 3u);
        m = (m << 1) | (v >> 2);
    }
    *code = static_cast<uint16_t>(c);
    *mask = static_cast<uint8_t>(m);
}

// The window of K bases that starts at base p of the tile: false when a break lies in it, else *fw = its 2K bits.
// Reads code words p / 16 .. + 2 and mask words p / 32, + 1 (they exist for every p below the tile's size; what they hold
// beyond the window is shifted out).
__device__ inline bool sc_window(const uint32_t* codes, const uint32_t* masks, uint32_t p, uint32_t K, uint64_t* fw) {
    const uint32_t w = p >> 4, s = 2u * (p & 15u);
    const uint64_t hi = (static_cast<uint64_t>(codes[w]) << 32) | codes[w + 1];
    const uint64_t x = s ? (hi << s) | (codes[w + 2] >> (32u - s)) : hi;
    *fw = x >> (64u - 2u * K);
    const uint32_t mw = p >> 5, t = p & 31u;
    const uint64_t mm = ((static_cast<uint64_t>(masks[mw]) << 32) | masks[mw + 1]) << t;
    return (mm >> (64u - K)) == 0;
}

// The tile walk over a read of L bases: the tile at base t0 holds *nb bases and the *nw window positions t0 .. t0 + *nw - 1;
// the next tile starts at t0 + *nw, K - 1 bases before this one's end.  false: no window from t0 on.
__device__ inline bool sc_tile(uint32_t t0, uint32_t L, uint32_t tile, uint32_t K, uint32_t* nb, uint32_t* nw) {
    if (L < K || t0 > L - K) return false;
    *nb = L - t0 < tile ? L - t0 : tile;
    *nw = *nb - K + 1;
    return true;
}

// A lane's walk over the reference's text, a byte at a time, from its first byte on (vk_fasta.h's FaWalk with a 2K-bit
// window and its reverse complement rolled along): the windows that START among the lane's own bytes.
struct ScWalk {
    uint64_t fw = 0, rc = 0;
    uint32_t run = 0;        // bases since the walk began or the last break
    uint32_t hdr = 0;        // inside a header line
    uint32_t ls = 0;         // the next byte starts a line
    uint32_t cr = 0;         // a '\r' of a sequence line waits for the byte behind it
    uint32_t extra = 0;      // bases taken behind the lane's own bytes

    // true: a window ends at this byte, *key is its key
    __device__ inline bool step(uint32_t b, bool owned, uint32_t K, uint64_t* key) {
        const bool nl = b == '\n';
        if (cr && !nl) run = 0;   // '\r' + '\n' is a line end; before anything else the '\r' is a byte like any other non-base
        if (ls) hdr = b == '>' ? 1u : 0u;
        if (ls && hdr) run = 0;   // a record ends at a header line
        ls = nl ? 1u : 0u;
        const bool seq = !nl && !hdr;
        cr = seq && b == '\r' ? 1u : 0u;
        if (!seq || cr) return false;
        const uint32_t c = sc_code(b);
        if (c > 3u) {
            run = 0;
            return false;
        }
        ++run;
        if (!owned) ++extra;
        const uint64_t mask = (1ull << (2u * K)) - 1u;
        fw = ((fw << 2) | c) & mask;
        rc = (rc >> 2) | (static_cast<uint64_t>(3u - c) << (2u * K - 2u));
        if (run < K) return false;
        *key = fw < rc ? fw : rc;
        return true;
    }

    // behind the lane's own bytes: windows are still open, or a '\r' still waits for its verdict
    __device__ inline bool more(uint32_t K) const { return (run > 0 || cr) && extra < K - 1; }
};

struct ScBuildOut {   // what a build leaves in its workspace (plain: vk_textplan.h sizes the workspace with it)
    unsigned long long windows, distinct;
    uint32_t full, pad;
};

#ifndef VK_SCREEN_LANE_ONLY

// ------------------------------------------------------------------ the set --

template <bool kInsert>
__global__ __launch_bounds__(kFaThreads) void vk_sc_build_kernel(const uint8_t* base, FaMeta m, const uint32_t* carry, uint32_t K,
                                                                 uint64_t* table, uint64_t nslots, ScBuildOut* out) {
    __shared__ uint32_t s_wave[kFaThreads / 64];
    uint64_t u0, u1;
    const uint32_t s = fa_locate(m, blockIdx.x, &u0, &u1);
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    if (text[0] != '>') return;   // VK_ST_BAD_START (a sample with a workgroup is not empty): no set
    uint32_t nwin = 0, nnew = 0, full = 0;
    for (uint64_t u = u0; u < u1; ++u) {
        uint32_t w[kFaLaneBytes / 4], n;
        uint64_t c0;
        fa_load(text, len, u, m.unit_bytes, w, &c0, &n);
        const bool first_ls = n && (c0 == 0 || text[c0 - 1] == '\n');
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        uint32_t total;
        const uint32_t excl = fa_block_excl_max(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, s_wave, &total);
        if (n == 0) continue;   // (uniform calls above; nothing below meets a barrier)
        ScWalk wk;
        wk.hdr = excl ? excl & 1u : carry[m.unit_first[s] + u];
        wk.ls = first_ls ? 1u : 0u;
        uint64_t p = c0;
        const uint64_t own_end = c0 + n;
        while (p < len && (p < own_end || wk.more(K))) {
            uint64_t key;
            if (wk.step(text[p], p < own_end, K, &key)) {
                ++nwin;
                if (kInsert) {
                    const uint32_t r = sc_insert(table, nslots, key);
                    nnew += r == 1u ? 1u : 0u;
                    full |= r == 2u ? 1u : 0u;
                }
            }
            ++p;
        }
    }
    // the sums: one per wave, one atomic each
    for (uint32_t d = 32; d; d >>= 1) {
        nwin += __shfl_down(nwin, d, 64);
        nnew += __shfl_down(nnew, d, 64);
        full |= __shfl_down(full, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (nwin) atomicAdd(&out->windows, static_cast<unsigned long long>(nwin));
        if (nnew) atomicAdd(&out->distinct, static_cast<unsigned long long>(nnew));
        if (full) atomicOr(&out->full, 1u);
    }
}

// ---------------------------------------------------------------- the screen --

struct ScParams {
    const uint64_t* table;
    uint64_t nslots;
    uint32_t K, min_hits, keep, tile;
};

__device__ inline void sc_wave_lds_fence() {
    // LDS operations of one wavefront execute in order; this only stops the compiler from moving LDS accesses across the point.
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline uint32_t sc_uniform(uint32_t v) {   // a value that every lane of the wave holds, as a scalar
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

// a record's bytes [r.h, end)
__device__ inline uint64_t sc_rec_end(const ClRec& r, const EmSample& s) { return r.qe == ~0ull ? s.off + s.len : r.qe + 1; }

__global__ void __launch_bounds__(kClThreads) vk_sc_match_kernel(const uint8_t* text, const EmSample* samples,
                                                                const uint64_t* rec_base, uint32_t nsamples, uint64_t nrec,
                                                                const ClRec* recs, const uint32_t* status, ScParams P,
                                                                uint64_t* out_bytes, unsigned long long* stats) {
    __shared__ uint32_t s_codes[kClThreads / 64][kScCodeWords];
    __shared__ uint32_t s_masks[kClThreads / 64][kScMaskWords];
    const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)));
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* codes = s_codes[wave];
    uint32_t* masks = s_masks[wave];
    uint16_t* codes16 = reinterpret_cast<uint16_t*>(codes);
    uint8_t* masks8 = reinterpret_cast<uint8_t*>(masks);
    const uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kScRecsPerBlock;
    // the wave's sums for the sample of its last record: flushed when the sample changes and at the end
    uint32_t cur = ~0u;
    unsigned long long n_in = 0, n_kept = 0, b_in = 0, b_kept = 0;
    for (uint32_t j = wave; j < kScRecsPerBlock; j += kClThreads / 64) {
        const uint64_t ri = r0 + j;
        if (ri >= nrec) break;
        const uint32_t si = cl_find_u64(rec_base, nsamples, ri);
        if (status[si] != 0) {
            if (lane == 0) out_bytes[ri] = 0;
            continue;
        }
        if (si != cur) {
            if (lane == 0 && cur != ~0u) {
                atomicAdd(stats + 4ull * cur + 0, n_in);
                atomicAdd(stats + 4ull * cur + 1, n_kept);
                atomicAdd(stats + 4ull * cur + 2, b_in);
                atomicAdd(stats + 4ull * cur + 3, b_kept);
            }
            cur = si;
            n_in = n_kept = b_in = b_kept = 0;
        }
        const EmSample s = samples[si];
        const ClRec r = recs[ri];
        const uint8_t* seq = text + r.he + 1;
        uint32_t L = static_cast<uint32_t>(r.se - r.he - 1);
        if (L && seq[L - 1] == '\r') --L;
        L = sc_uniform(L);   // (a scalar: the tile loop is the wave's)
        uint32_t hits = 0, t0 = 0, nb, nw;
        while (hits < P.min_hits && sc_tile(t0, L, P.tile, P.K, &nb, &nw)) {
            sc_wave_lds_fence();   // (the windows of the tile before are read)
            for (uint32_t c = lane; c < (nb + 7u) / 8u; c += 64) {
                uint16_t code;
                uint8_t mask;
                sc_pack8(seq + t0 + 8u * c, min(8u, nb - 8u * c), &code, &mask);
                codes16[c ^ 1u] = code;
                masks8[c ^ 3u] = mask;
            }
            sc_wave_lds_fence();
            for (uint32_t p0 = 0; p0 < nw && hits < P.min_hits; p0 += 64) {
                const uint32_t p = p0 + lane;
                bool hit = false;
                if (p < nw) {
                    uint64_t fw;
                    if (sc_window(codes, masks, p, P.K, &fw)) hit = sc_probe(P.table, P.nslots, sc_key(fw, P.K));
                }
                // (the sum is the wave's: kept in a scalar register, so that the loops around it stay the wave's own)
                hits = sc_uniform(hits + static_cast<uint32_t>(__popcll(__ballot(hit))));
            }
            t0 = sc_uniform(t0 + nw);
        }
        const bool match = hits >= P.min_hits;
        const bool kept = match == (P.keep != 0);
        ++n_in;
        b_in += L;
        if (kept) {
            ++n_kept;
            b_kept += L;
        }
        if (lane == 0) out_bytes[ri] = kept ? sc_rec_end(r, s) - r.h : 0;
    }
    if (lane == 0 && cur != ~0u) {
        atomicAdd(stats + 4ull * cur + 0, n_in);
        atomicAdd(stats + 4ull * cur + 1, n_kept);
        atomicAdd(stats + 4ull * cur + 2, b_in);
        atomicAdd(stats + 4ull * cur + 3, b_kept);
    }
}

__global__ void __launch_bounds__(kClThreads) vk_sc_write_kernel(const uint8_t* text, const uint64_t* rec_base,
                                                                const uint64_t* out_offs, uint32_t nsamples, uint64_t nrec,
                                                                const ClRec* recs, const uint64_t* prefix, uint8_t* out) {
    const uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kScRecsPerBlock;
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (uint32_t j = wave; j < kScRecsPerBlock; j += kClThreads / 64) {
        const uint64_t ri = r0 + j;
        if (ri >= nrec) break;
        const uint64_t at = prefix[ri], n = prefix[ri + 1] - at;
        if (n == 0) continue;   // (the record goes, or its sample has a status)
        const uint32_t si = cl_find_u64(rec_base, nsamples, ri);
        const uint8_t* src = text + recs[ri].h;
        uint8_t* o = out + out_offs[si] + (at - prefix[rec_base[si]]);
        for (uint64_t i = lane; i < n; i += 64) o[i] = src[i];
    }
}

__global__ void __launch_bounds__(kClThreads) vk_sc_pad_kernel(const uint64_t* rec_base, const uint64_t* out_offs,
                                                              uint32_t nsamples, const uint64_t* prefix, uint8_t* out,
                                                              uint64_t* out_lengths) {
    const uint32_t si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= nsamples) return;
    const uint64_t n = prefix[rec_base[si + 1]] - prefix[rec_base[si]], end = (n + 15) / 16 * 16;
    out_lengths[si] = n;
    for (uint64_t i = n; i < end; ++i) out[out_offs[si] + i] = 0;
}

#endif  // VK_SCREEN_LANE_ONLY

}  // namespace

#endif  // VK_SCREEN_H
