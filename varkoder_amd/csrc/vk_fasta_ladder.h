// vk_fasta_ladder.h -- a subsample ladder drawn from FASTA text in HBM: `image --from-fasta --fragments`
// (vk_count_fasta_sampled_device).  Part of the one translation unit vkimg.hip, on top of vk_fasta.h: the same cut by
// bytes (lanes of kFaLaneBytes, units, spans of units), the same header-state kernels, the same rule for what a base is.
//
// The rule ("--from-fasta --fragments"; tests/fasta_ladder_ref.py is the same rule in Python): the joined
// bytes of a sample's records, in order, have ORDINALS 0 .. bases - 1.  A step of the ladder has a seed, a threshold and
// a shift; the fragment of ordinal q is (q + shift) div L; fragment f is taken iff sample_hash(seed, f) < threshold.  A
// window counts iff it counts in the whole count, its first and last byte lie in one fragment, and that one is taken.
//
// An assembly has no reads, so nothing in the text says where a fragment starts: a lane needs the ORDINAL of its first
// byte, a plain (not segmented) prefix sum of sequence bytes.
//   vk_fa_summary_kernel, vk_fa_scan_kernel   (vk_fasta.h) the header state that enters every unit
//   vk_fa_ord_kernel       per lane: its sequence bytes, scanned over the unit -> the INDEX, a u32 per lane (ordinal
//                          relative to the unit | the header state and line start at its first byte), and a u64 per unit
//   vk_fa_ordscan_kernel   workgroup per sample: the units' sums scanned in place; the sample's bases
//   vk_fa_frag_count_kernel<K>   a workgroup per (pair, span of units): a lane reads its index word (4 bytes for 64 of
//                          text), hashes the fragments its own bytes fall in, and if none is taken neither loads nor
//                          walks its text.  A lane that walks tracks (q + shift) mod L and the fragment number byte by
//                          byte: one 64-bit division per lane.
// The index is 1/16 of the text and lives in the context's workspace for the call.  Histograms as in vk_fa_count_kernel:
// LDS per workgroup for k <= 7, global atomics on the pair's row for k = 8, 9; runs of one code folded (poly-A).
// The lane-local code (fa_lane_bases, FaFragWalk) compiles for the host: tests/emul/fasta_ladder_emul.cpp.
#ifndef VK_FASTA_LADDER_H
#define VK_FASTA_LADDER_H

#include "vk_lane.h"
#include "vk_fasta.h"

namespace {

// a lane's word of the index
constexpr uint32_t kFaIdxHdr = 1u << 31;          // its first byte lies in a header line (unless it starts a line itself)
constexpr uint32_t kFaIdxLs = 1u << 30;           // its first byte starts a line
constexpr uint32_t kFaIdxOrd = kFaIdxLs - 1u;     // sequence bytes of the unit before it

// Sequence bytes (joined bytes, every class) among a lane's n bytes.  hdr, first_ls: the state at its first byte; next:
// the byte behind its last one, '\n' at the sample's end (a '\r' before a line end or as the last byte is no sequence).
__device__ inline uint32_t fa_lane_bases(const uint32_t* w, uint32_t n, uint32_t hdr, bool first_ls, uint32_t next) {
    uint32_t nb = 0;
    bool ls = first_ls;
#pragma unroll
    for (uint32_t i = 0; i < kFaLaneBytes; ++i) {
        if (i < n) {
            const uint32_t b = fa_byte(w, i);
            const uint32_t nx = i + 1 < kFaLaneBytes && i + 1 < n ? fa_byte(w, (i + 1) & (kFaLaneBytes - 1)) : next;
            hdr = ls ? (b == '>' ? 1u : 0u) : hdr;
            ls = b == '\n';
            nb += !ls && !hdr && !(b == '\r' && nx == '\n') ? 1u : 0u;
        }
    }
    return nb;
}

struct FaFrag {   // one step of the ladder
    uint64_t seed, threshold, shift;
    uint32_t len;   // L
};

// FaWalk with the ordinal of every sequence byte: where it lies in its fragment (r), which fragment (f), whether that one
// is taken (tk).  `taken`: the lane's own sequence bytes in taken fragments.
struct FaFragWalk {
    uint32_t code = 0, run = 0, hdr = 0, ls = 0, cr = 0, cr_owned = 0, extra = 0;   // as FaWalk's
    uint32_t pend_code = 0, pend_n = 0;
    uint64_t f = 0;
    uint32_t r = 0, tk = 0;
    uint32_t taken = 0;

    // q: the ordinal of the first sequence byte the walk will meet
    __device__ inline void start(const FaFrag& s, uint64_t q) {
        const uint64_t t = q + s.shift;
        f = t / s.len;
        r = static_cast<uint32_t>(t - f * s.len);
        tk = vkl::sample_take(s.seed, f, s.threshold) ? 1u : 0u;
    }

    // Is any fragment taken that holds one of the n ordinals from the start on?  (n: no less than the lane's sequence
    // bytes; its own byte count will do.)
    __device__ inline bool any_taken(const FaFrag& s, uint32_t n) const {
        if (n == 0) return false;
        if (tk) return true;
        uint64_t g = f;
        for (uint64_t rem = static_cast<uint64_t>(r) + n; rem > s.len; rem -= s.len)
            if (vkl::sample_take(s.seed, ++g, s.threshold)) return true;
        return false;
    }

    __device__ inline void advance(const FaFrag& s) {
        if (++r == s.len) {
            r = 0;
            ++f;
            tk = vkl::sample_take(s.seed, f, s.threshold) ? 1u : 0u;
        }
    }

    template <int K, class Add>
    __device__ inline void step(uint32_t b, bool owned, const FaFrag& s, Add& add) {
        const bool nl = b == '\n';
        if (cr && !nl) {   // the '\r' before this byte was a sequence byte after all: a non-base with an ordinal
            taken += cr_owned & tk;
            run = 0;
            advance(s);
        }
        hdr = ls ? (b == '>' ? 1u : 0u) : hdr;
        run = ls && hdr ? 0u : run;
        ls = nl ? 1u : 0u;
        const bool seq = !nl && !hdr;
        const bool is_cr = seq && b == '\r';
        cr = is_cr ? 1u : 0u;
        cr_owned = is_cr ? (owned ? 1u : 0u) : cr_owned;
        const bool counted = seq && !is_cr;
        taken += counted && owned ? tk : 0u;
        const uint32_t c = fa_code(b);
        const bool base = counted && c <= 3u;
        run = counted ? (base ? run + 1u : 0u) : run;
        code = base ? ((code << 2) | c) & ((1u << (2 * K)) - 1u) : code;
        extra += base && !owned ? 1u : 0u;
        // the window's K bytes lie in one fragment iff its last byte is at least K - 1 into it
        const bool emit = base && run >= static_cast<uint32_t>(K) && r >= static_cast<uint32_t>(K - 1) && tk;
        const bool same = pend_n && pend_code == code;
        if (emit && !same && pend_n) add(pend_code, pend_n);
        pend_n = emit ? (same ? pend_n + 1u : 1u) : pend_n;
        pend_code = emit ? code : pend_code;
        if (counted) advance(s);
    }

    template <int K>
    __device__ inline bool more() const { return (run > 0 || cr) && extra < static_cast<uint32_t>(K - 1); }

    template <class Add>
    __device__ inline void flush(Add& add) {
        if (pend_n) add(pend_code, pend_n);
        pend_n = 0;
    }
};

struct FaPairs {
    const uint64_t* sample;      // [npairs] the pair's sample
    const uint64_t* seed;        // [npairs]
    const uint64_t* threshold;   // [npairs]
    const uint64_t* shift;       // [npairs]
    const uint64_t* wg_first;    // [npairs + 1] first workgroup of each pair
    uint32_t npairs, frag_len;
};

#ifndef VK_FASTA_LANE_ONLY

// Exclusive sum of v over the lanes of the workgroup, in lane order (all kFaThreads lanes call it); *total = the sum of
// all.  s_wave: kFaThreads / 64 elements of LDS.
template <class T>
__device__ inline T fa_block_excl_sum(T v, T* s_wave, T* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    T excl = inc - v;
    __syncthreads();
    T all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kFaThreads / 64; ++i) {
        const T t = s_wave[i];
        if (i < wave) excl += t;
        all += t;
    }
    __syncthreads();   // (s_wave is written again by the next call)
    *total = all;
    return excl;
}

// The index: lane_idx[(unit_first[s] + u) * (unit_bytes / kFaLaneBytes) + lane], unit_ord[unit_first[s] + u] = the unit's
// sequence bytes (vk_fa_ordscan_kernel turns them into the ordinal of the unit's first byte).
__global__ __launch_bounds__(kFaThreads) void vk_fa_ord_kernel(const uint8_t* base, FaMeta m, const uint32_t* carry, uint32_t* lane_idx,
                                                               unsigned long long* unit_ord) {
    __shared__ uint32_t s_wave[kFaThreads / 64];
    uint64_t u0, u1;
    const uint32_t s = fa_locate(m, blockIdx.x, &u0, &u1);
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    const uint32_t lanes = m.unit_bytes / kFaLaneBytes;
    for (uint64_t u = u0; u < u1; ++u) {
        uint32_t w[kFaLaneBytes / 4], n;
        uint64_t c0;
        fa_load(text, len, u, m.unit_bytes, w, &c0, &n);
        const bool first_ls = n && (c0 == 0 || text[c0 - 1] == '\n');
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        uint32_t total;
        const uint32_t excl = fa_block_excl_max(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, s_wave, &total);
        const uint64_t unit = m.unit_first[s] + u;
        const uint32_t hdr = excl ? excl & 1u : carry[unit];
        const uint32_t next = n && c0 + n < len ? text[c0 + n] : '\n';
        const uint32_t nb = n ? fa_lane_bases(w, n, hdr, first_ls, next) : 0u;
        const uint32_t before = fa_block_excl_sum(nb, s_wave, &total);
        if (threadIdx.x < lanes) lane_idx[unit * lanes + threadIdx.x] = before | (hdr ? kFaIdxHdr : 0u) | (first_ls ? kFaIdxLs : 0u);
        if (threadIdx.x == 0) unit_ord[unit] = total;
    }
}

__global__ __launch_bounds__(kFaThreads) void vk_fa_ordscan_kernel(const uint8_t* base, FaMeta m, unsigned long long* unit_ord,
                                                                   unsigned long long* bases) {
    __shared__ unsigned long long s_wave[kFaThreads / 64];
    const uint32_t s = blockIdx.x;
    const uint64_t first = m.unit_first[s], nunits = m.unit_first[s + 1] - first;
    unsigned long long running = 0;
    for (uint64_t t = 0; t < nunits; t += kFaThreads) {
        const uint64_t u = t + threadIdx.x;
        const unsigned long long v = u < nunits ? unit_ord[first + u] : 0ull;
        unsigned long long total;
        const unsigned long long excl = fa_block_excl_sum(v, s_wave, &total);
        if (u < nunits) unit_ord[first + u] = running + excl;
        running += total;
    }
    // (a sample with VK_ST_BAD_START is not read: zero bases, as vk_fa_count_kernel leaves them)
    if (threadIdx.x == 0) bases[s] = m.lens[s] && base[m.offs[s]] != '>' ? 0ull : running;
}

// The lane's 64 bytes at `at` (< len) of a sample (16-byte loads that begin below len).
__device__ inline void fa_load_lane(const uint8_t* text, uint64_t len, uint64_t at, uint32_t* w) {
#pragma unroll
    for (uint32_t j = 0; j < kFaLaneBytes / 16; ++j) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (at + 16u * j < len) v = *reinterpret_cast<const uint4*>(text + at + 16u * j);
        w[4 * j + 0] = v.x;
        w[4 * j + 1] = v.y;
        w[4 * j + 2] = v.z;
        w[4 * j + 3] = v.w;
    }
}

template <int K>
__global__ __launch_bounds__(kFaThreads) void vk_fa_frag_count_kernel(const uint8_t* base, FaMeta m, FaPairs ps, const uint32_t* lane_idx,
                                                                      const unsigned long long* unit_ord, uint32_t* hist,
                                                                      unsigned long long* taken) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    constexpr bool LDSH = K <= 7;
    __shared__ uint32_t s_hist[LDSH ? NCODE : 1];
    uint32_t lo = 0, hi = ps.npairs;   // the last pair whose first workgroup is <= this one
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ps.wg_first[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    const uint32_t p = lo, s = static_cast<uint32_t>(ps.sample[p]);
    const uint64_t first = m.unit_first[s], nunits = m.unit_first[s + 1] - first;
    const uint64_t u0 = (blockIdx.x - ps.wg_first[p]) * m.span_units;
    const uint64_t u1 = u0 + m.span_units < nunits ? u0 + m.span_units : nunits;
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    if (text[0] != '>') return;   // VK_ST_BAD_START (a sample with a workgroup is not empty): zero histograms, nothing taken
    uint32_t* row = hist + static_cast<size_t>(p) * NCODE;
    if (LDSH) {
        for (uint32_t i = threadIdx.x; i < NCODE; i += kFaThreads) s_hist[i] = 0;
        __syncthreads();
    }
    FaAdd<K> add{LDSH ? s_hist : row};
    const FaFrag st{ps.seed[p], ps.threshold[p], ps.shift[p], ps.frag_len};
    const uint32_t lanes = m.unit_bytes / kFaLaneBytes;
    uint32_t my_taken = 0;
    int walked = 0;
    for (uint64_t u = u0; u < u1; ++u) {   // (no barrier inside)
        const uint64_t c0 = u * m.unit_bytes + static_cast<uint64_t>(threadIdx.x) * kFaLaneBytes;
        if (threadIdx.x >= lanes || c0 >= len) continue;
        const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
        const uint32_t word = lane_idx[(first + u) * lanes + threadIdx.x];
        FaFragWalk wk;
        wk.start(st, unit_ord[first + u] + (word & kFaIdxOrd));
        if (!wk.any_taken(st, n)) continue;   // neither loaded nor walked
        wk.hdr = word & kFaIdxHdr ? 1u : 0u;
        wk.ls = word & kFaIdxLs ? 1u : 0u;
        uint32_t w[kFaLaneBytes / 4];
        fa_load_lane(text, len, c0, w);
#pragma unroll
        for (uint32_t i = 0; i < kFaLaneBytes; ++i)
            if (i < n) wk.template step<K>(fa_byte(w, i), true, st, add);
        for (uint64_t q = c0 + n; q < len && wk.template more<K>(); ++q) wk.template step<K>(text[q], false, st, add);
        wk.flush(add);
        my_taken += wk.taken;
        walked = 1;
    }
    // the step's taken bytes: a sum per wave, one atomic each
    for (uint32_t d = 32; d; d >>= 1) my_taken += __shfl_down(my_taken, d, 64);
    if ((threadIdx.x & 63u) == 0 && my_taken) atomicAdd(taken + p, static_cast<unsigned long long>(my_taken));
    if (LDSH) {
        if (!__syncthreads_or(walked)) return;   // (uniform: nobody added anything)
        for (uint32_t i = threadIdx.x; i < NCODE; i += kFaThreads) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(row + i, v);
        }
    }
}

#endif  // VK_FASTA_LANE_ONLY

}  // namespace

#endif  // VK_FASTA_LADDER_H
