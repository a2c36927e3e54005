// vk_adapter.h -- adapters by sequence in step B (`image --from-raw --detect-adapters / --adapter-sequence`):
// detection of a group's adapter from its first reads, and fastp's trimBySequence inside vk_cl_clean_kernel.
// Part of the one translation unit vkimg.hip, after vk_clean.h (device code for gfx950; see the notes there).
//
// The rules are this project's contract, modelled on fastp 0.23 ("Step B"); tests/adapter_ref.py is
// the same contract in Python and the GPU must equal it byte for byte.  A group is R1, R2 or the single reads of a
// sample; its evaluation set is its first min(262144, budgeted) records.
//
// Launch sequence of vk_clean_detect_device, after vk_clean.h's record index over the evaluation sets, per slice of
// at most kAdSlice groups:
//   vk_ad_hist_kernel     lane per record: every ACGT 10-mer at read positions 20 <= p <= len - 10 that passes the
//                         key filters into the group's 4^10 u32 table (global atomics)
//   vk_ad_top_kernel      workgroup per group: `total`, each lane's top 10 in registers, then 10
//                         rounds of a workgroup maximum -> the ranked keys (count << 20 | ~key) and `total`
//   (host)                the candidates (fold over 20) and room for their occurrences
//   vk_ad_collect_kernel  lane per record again: the occurrences of the group's candidates at 20 <= p <=
//                         len - 10 - shiftTail into each candidate's list
//   vk_ad_extend_kernel   workgroup per (group, candidate): backward, then forward, one step at a time -- the live
//                         occurrences vote their byte in LDS, the workgroup decides, a state per occurrence
//   (host)                a seed with fewer than 50 occurrences is skipped; else D = reverse(backward) + seed +
//                         forward, snapped to a listed adapter or accepted when both directions ran out; the first
//                         accepted candidate is the group's adapter
#ifndef VK_ADAPTER_H
#define VK_ADAPTER_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr uint32_t kAdEval = 262144;        // records of a group that detection reads
constexpr uint32_t kAdK = 10;               // seed length
constexpr uint32_t kAdKeys = 1u << (2 * kAdK);
constexpr uint32_t kAdFrom = 20;            // first read position of a counted window
constexpr uint32_t kAdTop = 10;             // candidates ranked per group
constexpr uint32_t kAdFold = 20;            // count * 4^10 / total must exceed this
constexpr uint32_t kAdMinVotes = 50;        // fewer live occurrences than this: the extension ran out
constexpr uint32_t kAdPct = 95;             // the top byte needs this share of the votes
constexpr uint32_t kAdMaxLen = 60;          // bases of a detected string kept
constexpr uint32_t kAdKeep = 64;            // bytes an extension keeps per direction (a ring for the backward one)
constexpr uint32_t kAdSlice = 32;           // groups per slice: 128 MiB of tables
constexpr uint32_t kAdThreads = 1024;       // threads of the per-group and per-candidate workgroups
constexpr uint32_t kAdMaxAdapter = kClMaxAdapter;
constexpr uint32_t kAdSnap = 16;            // bases of a listed adapter that a detected string must hold to snap to it

// the listed adapters, in snapping order (the table of varkoder_amd/adapters.py; a CPU test holds the two equal)
constexpr const char* kAdKnown[] = {
    "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA",   // Illumina TruSeq read 1
    "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT",   // Illumina TruSeq read 2
    "CTGTCTCTTATACACATCT",                 // Nextera / Tn5
    "TGGAATTCTCGGGTGCCAAGG",               // Illumina small RNA 3'
};

struct AdGroup {         // a group of a detection: its evaluation set is records [rec0, rec0 + n) of the index
    uint64_t rec0, n;
};

struct AdCand {          // a candidate seed and its occurrence list (cap 0: no candidate in this rank)
    uint32_t key, cap;
    uint64_t off;
};

struct AdOcc {           // an occurrence of a seed: text offset of its first base, steps each way it may take
    uint64_t at;
    uint32_t fwd, back;
};

struct AdExt {           // an extension's result: steps taken, 1 backward ran out | 2 forward ran out, occurrences, the bytes
    uint32_t nb, nf, flags, nocc;
    uint8_t back[kAdKeep];   // backward byte j at [j % kAdKeep]
    uint8_t fwd[kAdKeep];    // forward byte j at [j] (j < kAdKeep)
};

__device__ inline uint32_t ad_code(uint8_t b) {   // A0 C1 G2 T3 (lexicographic: key order is string order); 4: other
    switch (b) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        default: return 4;
    }
}

__device__ inline bool ad_key_ok(uint32_t key) {
    if (key == 0 || (key >> 12) == 0xAAu) return false;   // A x 10; a GGGG head
    uint32_t per = 0;                                       // four 8-bit base counters
    for (uint32_t i = 0; i < kAdK; ++i) per += 1u << (8 * ((key >> (2 * i)) & 3u));
    const uint32_t a = per & 255u, c = (per >> 8) & 255u, g = (per >> 16) & 255u, t = per >> 24;
    return a < 6 && c < 6 && g < 6 && t < 6 && c + g < 8;
}

// the group of slice-local record t: (group, record in the index)
__device__ inline uint32_t ad_group_of(const uint64_t* gbase, uint32_t ng, uint64_t t) { return cl_find_u64(gbase, ng, t); }

__global__ void __launch_bounds__(kClThreads) vk_ad_hist_kernel(const uint8_t* text, const ClRec* recs, const AdGroup* groups,
                                                               const uint64_t* gbase, uint32_t ng, uint32_t* hist) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= gbase[ng]) return;
    const uint32_t g = ad_group_of(gbase, ng, t);
    const ClRec r = recs[groups[g].rec0 + (t - gbase[g])];
    if (!cl_rec_ok(text, r)) return;
    const uint8_t* s = text + r.he + 1;
    const uint64_t len = r.se - r.he - 1;
    uint32_t* h = hist + static_cast<uint64_t>(g) * kAdKeys;
    uint32_t key = 0, run = 0;
    for (uint64_t i = 0; i < len; ++i) {   // window [i + 1 - 10, i]: counted from p = 20, i.e. i >= 29
        const uint32_t c = ad_code(s[i]);
        run = c < 4 ? run + 1 : 0;
        key = ((key << 2) | (c & 3u)) & (kAdKeys - 1);
        // (only keys that pass the filters: a dropped key is never ranked, and poly-G or poly-A runs would otherwise
        // send every lane of a wave to one hot counter)
        if (run >= kAdK && i + 1 >= kAdFrom + kAdK && ad_key_ok(key)) atomicAdd(h + key, 1u);
    }
}

// workgroup maximum (op 0) or sum (op 1) of one u64 per thread through LDS; every thread gets the result
__device__ inline uint64_t ad_block_reduce(uint64_t v, uint64_t* sh, bool sum) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const uint64_t o = sh[threadIdx.x + s];
            sh[threadIdx.x] = sum ? sh[threadIdx.x] + o : max(sh[threadIdx.x], o);
        }
        __syncthreads();
    }
    const uint64_t r = sh[0];
    __syncthreads();
    return r;
}

// ranked[g][i] = count << 20 | (4^10 - 1 - key) of the i-th key (0: none), totals[g] = the filtered keys' count sum
__global__ void __launch_bounds__(kAdThreads) vk_ad_top_kernel(const uint32_t* hist, uint64_t* ranked, uint64_t* totals) {
    __shared__ uint64_t sh[kAdThreads];
    const uint32_t g = blockIdx.x;
    const uint32_t* h = hist + static_cast<uint64_t>(g) * kAdKeys;
    uint64_t top[kAdTop];
#pragma unroll
    for (uint32_t i = 0; i < kAdTop; ++i) top[i] = 0;
    uint64_t total = 0;
    for (uint32_t key = threadIdx.x; key < kAdKeys; key += kAdThreads) {
        const uint32_t c = h[key];
        if (c == 0) continue;   // (the histogram holds only keys that pass the filters)
        total += c;
        uint64_t v = (static_cast<uint64_t>(c) << 20) | (kAdKeys - 1 - key);   // larger: more often, then smaller key
        if (v > top[kAdTop - 1]) {
#pragma unroll
            for (uint32_t i = 0; i < kAdTop; ++i) {
                const uint64_t hi = max(v, top[i]);
                v = min(v, top[i]);
                top[i] = hi;
            }
        }
    }
    total = ad_block_reduce(total, sh, true);
    for (uint32_t i = 0; i < kAdTop; ++i) {
        const uint64_t best = ad_block_reduce(top[0], sh, false);
        if (best != 0 && top[0] == best) {   // (keys are distinct: one thread holds it) pop the head
#pragma unroll
            for (uint32_t j = 0; j + 1 < kAdTop; ++j) top[j] = top[j + 1];
            top[kAdTop - 1] = 0;
        }
        if (threadIdx.x == 0) ranked[static_cast<uint64_t>(g) * kAdTop + i] = best;
    }
    if (threadIdx.x == 0) totals[g] = total;
}

__global__ void __launch_bounds__(kClThreads) vk_ad_collect_kernel(const uint8_t* text, const ClRec* recs,
                                                                  const AdGroup* groups, const uint64_t* gbase, uint32_t ng,
                                                                  const AdCand* cands, uint32_t shift_tail,
                                                                  uint32_t* counts, AdOcc* occ) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= gbase[ng]) return;
    const uint32_t g = ad_group_of(gbase, ng, t);
    const ClRec r = recs[groups[g].rec0 + (t - gbase[g])];
    if (!cl_rec_ok(text, r)) return;
    uint32_t seeds[kAdTop];   // ~0: no candidate (a key has 20 bits)
#pragma unroll
    for (uint32_t c = 0; c < kAdTop; ++c) {
        const AdCand cd = cands[g * kAdTop + c];
        seeds[c] = cd.cap ? cd.key : ~0u;
    }
    const uint8_t* s = text + r.he + 1;
    const uint64_t len = r.se - r.he - 1;
    uint32_t key = 0, run = 0;
    for (uint64_t i = 0; i < len; ++i) {   // window p = i + 1 - 10: 20 <= p and p + 10 + shiftTail <= len
        const uint32_t cd = ad_code(s[i]);
        run = cd < 4 ? run + 1 : 0;
        key = ((key << 2) | (cd & 3u)) & (kAdKeys - 1);
        if (run < kAdK || i + 1 < kAdFrom + kAdK || i + 1 + shift_tail > len) continue;
        const uint64_t p = i + 1 - kAdK;
#pragma unroll
        for (uint32_t c = 0; c < kAdTop; ++c) {
            if (seeds[c] != key) continue;
            const uint32_t gc = g * kAdTop + c;
            const uint32_t at = atomicAdd(counts + gc, 1u);
            const AdCand cand = cands[gc];
            if (at < cand.cap)
                occ[cand.off + at] = AdOcc{r.he + 1 + p, static_cast<uint32_t>(len - shift_tail - (p + kAdK)),
                                           static_cast<uint32_t>(p)};
        }
    }
}

// one direction of an extension (dir 0 backward, 1 forward); returns true when it ran out.  state[i]: 0 dropped,
// 1 live, 2 + b: live and voted b at the last step (checked against that step's choice at the next one)
__device__ inline bool ad_extend_dir(const uint8_t* text, const AdOcc* occ, uint16_t* state, uint32_t n, uint32_t dir,
                                     uint32_t* votes, uint64_t* sh, uint8_t* keep, uint32_t* steps) {
    uint64_t most = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kAdThreads) {
        state[i] = 1;
        most = max(most, static_cast<uint64_t>(dir ? occ[i].fwd : occ[i].back));
    }
    most = ad_block_reduce(most, sh, false);   // (and the states are written before the first step reads them)
    uint32_t prev = 0;
    for (uint32_t j = 0; j <= most; ++j) {      // at j = most no occurrence has a byte left: the loop always ends
        if (threadIdx.x < 256) votes[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += kAdThreads) {
            uint32_t st = state[i];
            if (st >= 2 && st - 2 != prev) st = 0;   // disagreed with the byte chosen at the last step
            if (st == 0) {
                state[i] = 0;
                continue;
            }
            const AdOcc o = occ[i];
            if ((dir ? o.fwd : o.back) <= j) {       // no byte at this step, nor later
                state[i] = 0;
                continue;
            }
            const uint8_t b = text[dir ? o.at + kAdK + j : o.at - 1 - j];
            atomicAdd(votes + b, 1u);
            state[i] = static_cast<uint16_t>(2 + b);
        }
        __syncthreads();
        const uint64_t v = threadIdx.x < 256 ? votes[threadIdx.x] : 0;
        const uint64_t nv = ad_block_reduce(v, sh, true);
        const uint64_t best = ad_block_reduce(threadIdx.x < 256 ? (v << 8) | (255u - threadIdx.x) : 0, sh, false);
        if (nv < kAdMinVotes) return true;
        if ((best >> 8) * 100 < kAdPct * nv) return false;
        prev = 255u - static_cast<uint32_t>(best & 255u);
        if (threadIdx.x == 0 && (dir == 0 || j < kAdKeep)) keep[dir ? j : j % kAdKeep] = static_cast<uint8_t>(prev);
        *steps = j + 1;
    }
    return true;
}

__global__ void __launch_bounds__(kAdThreads) vk_ad_extend_kernel(const uint8_t* text, const AdCand* cands,
                                                                 const uint32_t* counts, const AdOcc* occ,
                                                                 uint16_t* state, AdExt* ext) {
    __shared__ uint64_t sh[kAdThreads];
    __shared__ uint32_t votes[256];
    __shared__ uint8_t keep[2][kAdKeep];
    const uint32_t gc = blockIdx.x;
    const AdCand cd = cands[gc];
    AdExt* e = ext + gc;
    if (cd.cap == 0) {
        if (threadIdx.x == 0) e->flags = e->nb = e->nf = e->nocc = 0;
        return;
    }
    const uint32_t n = min(counts[gc], cd.cap);
    uint32_t nb = 0, nf = 0;
    const bool back_out = ad_extend_dir(text, occ + cd.off, state + cd.off, n, 0, votes, sh, keep[0], &nb);
    __syncthreads();
    const bool fwd_out = ad_extend_dir(text, occ + cd.off, state + cd.off, n, 1, votes, sh, keep[1], &nf);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * kAdKeep; i += kAdThreads) {
        if (i < kAdKeep) e->back[i] = keep[0][i]; else e->fwd[i - kAdKeep] = keep[1][i - kAdKeep];
    }
    if (threadIdx.x == 0) {
        e->nb = nb;
        e->nf = nf;
        e->flags = (back_out ? 1u : 0u) | (fwd_out ? 2u : 0u);
        e->nocc = n;
    }
}

// ------------------------------------------------------------ trimming --

struct AdWin {           // 64 positions as ClWin holds 50: codes and non-ACGT flags at the even bits
    uint64_t lo, hi, nlo, nhi;
};

__device__ inline void ad_push(AdWin& w, const uint8_t* p, uint32_t i, uint32_t len) {   // drop position 0, append p[i] (or nothing) at 63
    const uint8_t b = i < len ? p[i] : 'A';
    const uint64_t c = (b >> 1) & 3u, bad = (i < len && !cl_acgt(b)) ? 1u : 0u;
    w.lo = (w.lo >> 2) | (w.hi << 62);
    w.hi = (w.hi >> 2) | (c << 62);
    w.nlo = (w.nlo >> 2) | (w.nhi << 62);
    w.nhi = (w.nhi >> 2) | (bad << 62);
}

__device__ inline uint64_t ad_even_mask(int n) {   // the even bits of the first n (0..32) positions
    constexpr uint64_t kEven = 0x5555555555555555ull;
    return n >= 32 ? kEven : n <= 0 ? 0ull : (((1ull << (2 * n)) - 1) & kEven);
}

// fastp's trimBySequence on p[0 .. rlen) with the adapter ad (ad->len > 0): the read's new length.  The adapter's
// window, shifted by -pos while pos < 0, is scored against the read's window at max(pos, 0): two ACGT codes by xor,
// an ACGT byte against a non-ACGT one always differs, two non-ACGT bytes are compared as they are
__device__ inline uint32_t cl_trim_seq(const uint8_t* p, uint32_t rlen, const ClAdapter* ad) {
    const int alen = static_cast<int>(ad->len);
    const int start = alen >= 16 ? -4 : alen >= 12 ? -3 : alen >= 8 ? -2 : 0;
    AdWin r = {};
    for (uint32_t i = 0; i < 64; ++i) ad_push(r, p, i, rlen);
    for (int pos = start; pos < static_cast<int>(rlen) - 4; ++pos) {
        const int cmplen = min(static_cast<int>(rlen) - pos, alen);
        const uint32_t s = pos < 0 ? static_cast<uint32_t>(-pos) : 0u;   // 0..4
        AdWin a{ad->lo, ad->hi, ad->nlo, ad->nhi};
        if (s) {
            a.lo = (a.lo >> (2 * s)) | (a.hi << (64 - 2 * s));
            a.hi >>= 2 * s;
            a.nlo = (a.nlo >> (2 * s)) | (a.nhi << (64 - 2 * s));
            a.nhi >>= 2 * s;
        }
        const int n = cmplen - static_cast<int>(s);   // positions compared
        const uint64_t vlo = ad_even_mask(n), vhi = ad_even_mask(n - 32);
        const uint64_t xl = a.lo ^ r.lo, xh = a.hi ^ r.hi;
        constexpr uint64_t kEven = 0x5555555555555555ull;
        const uint64_t ml = (xl | (xl >> 1)) & kEven, mh = (xh | (xh >> 1)) & kEven;
        uint32_t mism = __popcll(ml & ~(a.nlo | r.nlo) & vlo) + __popcll(mh & ~(a.nhi | r.nhi) & vhi) +
                        __popcll((a.nlo ^ r.nlo) & vlo) + __popcll((a.nhi ^ r.nhi) & vhi);
        uint64_t both_lo = a.nlo & r.nlo & vlo, both_hi = a.nhi & r.nhi & vhi;
        const uint32_t at = pos > 0 ? static_cast<uint32_t>(pos) : 0u;
        while (both_lo | both_hi) {   // (rare: a non-ACGT byte in the adapter and in the read at the same place)
            const uint32_t k = both_lo ? __builtin_ctzll(both_lo) / 2 : 32 + __builtin_ctzll(both_hi) / 2;
            if (both_lo) both_lo &= both_lo - 1; else both_hi &= both_hi - 1;
            if (ad->seq[k + s] != p[at + k]) ++mism;
        }
        if (mism <= static_cast<uint32_t>(cmplen) / 8) return at;
        if (pos >= 0) ad_push(r, p, static_cast<uint32_t>(pos) + 64, rlen);
    }
    return rlen;
}

// trimming by sequence of a read that the clean kernel keeps as p[0 .. len): its new length; a cut read is counted
__device__ inline uint32_t cl_seq_cut(const uint8_t* p, uint32_t len, const ClAdapter* ad, uint32_t* nread,
                                      uint32_t* nbase) {
    if (ad->len == 0) return len;
    const uint32_t n = cl_trim_seq(p, len, ad);
    if (n < len) {
        *nread += 1;
        *nbase += len - n;
    }
    return n;
}

}  // namespace

#endif  // VK_ADAPTER_H
