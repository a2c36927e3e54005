// vk_fasta.h -- k-mer counts (k = 5..9) straight from FASTA text in HBM: `image / query --from-fasta`, the dsk shim on a
// FASTA `-file`.  Part of the one translation unit vkimg.hip (device code for gfx950).  The dense k <= 7 kernel and the
// k = 8, 9 spill route of vk_count.h are FASTQ-shaped (four-line records, line phase) and are not used or touched here.
//
// The rule ("--from-fasta"; tests/fasta_ref.py is the same rule in Python): a line ends at '\n', a '\r'
// directly before it (or as the sample's last byte) belongs to the line end; a line whose first byte is '>' is a header
// line, none of its bytes are sequence; every other line's bytes, line ends removed, join into the current record.  A
// window of k bytes out of ACGTacgt counts; it runs across line ends, never across a header line or any other byte.
//
// Work is cut by BYTES, never by records (a record may be hundreds of megabases): a lane owns kFaLaneBytes of text, a
// unit is up to kFaThreads lanes (VKIMG_FASTA_UNIT_BYTES shrinks it), a workgroup runs over a span of consecutive units
// of one sample.
//   * Header state.  Whether a byte lies in a header line is a property of the start of its line, which may be any
//     distance back.  Nobody walks back: every lane states (has a line start, is its LAST line start a header), an
//     exclusive scan over the lanes of the unit (wave shuffles, the wave totals through LDS) gives each lane the state
//     at its first byte, and what comes in from before the unit is the same pair per unit, scanned across the units of
//     the sample by a kernel of its own:
//         vk_fa_summary_kernel   the pair of every unit
//         vk_fa_scan_kernel      workgroup per sample: the state that enters every unit; the sample's status word
//         vk_fa_count_kernel<K>  the count
//     (The first line end of a unit needs no stating: a lane that starts inside a header line sees it as it walks.)
//   * Windows across seams.  A lane owns the windows that START in its bytes.  Its rolling window starts empty at its
//     first byte; behind its last byte it reads on, through line ends, for the k - 1 further bases its open windows
//     need, and stops at a header line, a non-base or the sample's end.  Nothing is carried in from behind.
//   * k <= 7: a 4^k u32 histogram in LDS per workgroup (ds_add_u32), flushed to the sample's row with global atomics;
//     k = 8, 9: global atomics on the row.  A lane folds a run of equal codes into one addition (poly-A).
// The lane-local code (FaWalk, fa_lane_key) compiles for the host: tests/emul/fasta_emul.cpp runs it, a lane at a time,
// against tests/fasta_ref.py.
#ifndef VK_FASTA_H
#define VK_FASTA_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr uint32_t kFaLaneBytes = 64;                         // text bytes of a lane: four 16-byte loads
constexpr uint32_t kFaThreads = 256;                          // lanes of a workgroup
constexpr uint32_t kFaUnitBytes = kFaLaneBytes * kFaThreads;  // a unit, unless VKIMG_FASTA_UNIT_BYTES shrinks it
constexpr uint32_t kFaSpanUnits = 32;                         // units a workgroup runs over (1 with the switch set)

__device__ inline uint32_t fa_code(uint32_t b) {   // A0 C1 G2 T3 in either case; 4: every other byte
    const uint32_t u = b & 0xDFu;                    // (equal to an upper-case letter only for that letter's two cases)
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

__device__ inline uint32_t fa_byte(const uint32_t* w, uint32_t i) { return (w[i >> 2] >> (8u * (i & 3u))) & 255u; }

// What a lane states about its n bytes (w: the bytes, little endian; first_ls: its first byte starts a line):
// 0 = no line starts here, else 2 | (the last line that starts here is a header line).
__device__ inline uint32_t fa_lane_key(const uint32_t* w, uint32_t n, bool first_ls) {
    uint32_t key = 0;
    bool ls = first_ls;
#pragma unroll
    for (uint32_t i = 0; i < kFaLaneBytes; ++i) {
        if (i < n) {
            const uint32_t b = fa_byte(w, i);
            if (ls) key = 2u | (b == '>' ? 1u : 0u);
            ls = b == '\n';
        }
    }
    return key;
}

// A lane's walk over the text, a byte at a time, from its first byte on.  `owned` bytes are the lane's own (they count
// towards `bases`); behind them the walk goes on with owned = false for as long as more() says.
struct FaWalk {
    uint32_t code = 0;       // the last bases, two bits each
    uint32_t run = 0;        // bases since the walk began or the last break
    uint32_t hdr = 0;        // inside a header line
    uint32_t ls = 0;         // the next byte starts a line
    uint32_t cr = 0;         // a '\r' of a sequence line waits for the byte behind it
    uint32_t cr_owned = 0;
    uint32_t extra = 0;      // bases taken behind the lane's own bytes
    uint32_t bases = 0;      // sequence bytes (joined bytes, every class) among the lane's own
    uint32_t pend_code = 0, pend_n = 0;   // additions of one code not yet made

    // (Written with selects, one branch around the addition: sixty-four of these are unrolled over a lane's registers, and
    // nested early returns there cost an EXEC mask each.)
    template <int K, class Add>
    __device__ inline void step(uint32_t b, bool owned, Add& add) {
        const bool nl = b == '\n';
        // '\r' + '\n' is a line end; before anything else the '\r' is a byte like any other non-base
        const bool cr_break = cr && !nl;
        bases += cr_break ? cr_owned : 0u;
        run = cr_break ? 0u : run;
        hdr = ls ? (b == '>' ? 1u : 0u) : hdr;
        run = ls && hdr ? 0u : run;   // a record ends at a header line
        ls = nl ? 1u : 0u;
        const bool seq = !nl && !hdr;                // a byte of a sequence line
        const bool is_cr = seq && b == '\r';
        cr = is_cr ? 1u : 0u;
        cr_owned = is_cr ? (owned ? 1u : 0u) : cr_owned;
        const bool counted = seq && !is_cr;          // a sequence byte, whatever its class
        bases += counted && owned ? 1u : 0u;
        const uint32_t c = fa_code(b);
        const bool base = counted && c <= 3u;
        run = counted ? (base ? run + 1u : 0u) : run;
        code = base ? ((code << 2) | c) & ((1u << (2 * K)) - 1u) : code;
        extra += base && !owned ? 1u : 0u;
        // a window that started among the lane's own bytes (extra <= K - 1)
        const bool emit = base && run >= static_cast<uint32_t>(K);
        const bool same = pend_n && pend_code == code;
        if (emit && !same && pend_n) add(pend_code, pend_n);
        pend_n = emit ? (same ? pend_n + 1u : 1u) : pend_n;
        pend_code = emit ? code : pend_code;
    }

    // behind the lane's own bytes: windows are still open, or a '\r' still waits for its verdict
    template <int K>
    __device__ inline bool more() const { return (run > 0 || cr) && extra < static_cast<uint32_t>(K - 1); }

    template <class Add>
    __device__ inline void flush(Add& add) {
        if (pend_n) add(pend_code, pend_n);
        pend_n = 0;
    }
};

struct FaMeta {
    const uint64_t* offs;        // [nsamples] byte offset of each sample (multiple of 16)
    const uint64_t* lens;        // [nsamples]
    const uint64_t* wg_first;    // [nsamples + 1] first workgroup of each sample
    const uint64_t* unit_first;  // [nsamples + 1] first unit of each sample (index into ukey / carry)
    uint32_t nsamples, unit_bytes, span_units;
};

#ifndef VK_FASTA_LANE_ONLY

// Exclusive running maximum of `key` over the lanes of the workgroup, in lane order (all kFaThreads lanes call it);
// *total = the maximum over all of them.  s_wave: kFaThreads / 64 words of LDS.
__device__ inline uint32_t fa_block_excl_max(uint32_t key, uint32_t* s_wave, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = key;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d && o > inc) inc = o;
    }
    if (lane == 63) s_wave[wave] = inc;
    uint32_t excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 0;
    __syncthreads();
    uint32_t all = 0;
#pragma unroll
    for (uint32_t v = 0; v < kFaThreads / 64; ++v) {
        const uint32_t t = s_wave[v];
        if (v < wave && t > excl) excl = t;
        if (t > all) all = t;
    }
    __syncthreads();   // (s_wave is written again by the next call)
    *total = all;
    return excl;
}

// The sample and the units [*u0, *u1) of workgroup `wg`.
__device__ inline uint32_t fa_locate(const FaMeta& m, uint64_t wg, uint64_t* u0, uint64_t* u1) {
    uint32_t lo = 0, hi = m.nsamples;   // the last sample whose first workgroup is <= wg
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (m.wg_first[mid] <= wg) lo = mid; else hi = mid;
    }
    const uint64_t nunits = m.unit_first[lo + 1] - m.unit_first[lo];
    const uint64_t a = (wg - m.wg_first[lo]) * m.span_units;
    *u0 = a;
    *u1 = a + m.span_units < nunits ? a + m.span_units : nunits;
    return lo;
}

// The lane's bytes of unit u of a sample of `len` bytes at `text` (16-byte aligned): *n of them from *c0 on, in w.
// 16-byte loads that begin below `len` (the buffer is readable up to the sample's 16-byte rounded end).
__device__ inline void fa_load(const uint8_t* text, uint64_t len, uint64_t u, uint32_t unit_bytes, uint32_t* w, uint64_t* c0,
                               uint32_t* n) {
    const uint64_t at = u * unit_bytes + static_cast<uint64_t>(threadIdx.x) * kFaLaneBytes;
    const bool active = threadIdx.x * kFaLaneBytes < unit_bytes && at < len;
    *c0 = at;
    *n = !active ? 0u : len - at < kFaLaneBytes ? static_cast<uint32_t>(len - at) : kFaLaneBytes;
#pragma unroll
    for (uint32_t j = 0; j < kFaLaneBytes / 16; ++j) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (active && at + 16u * j < len) v = *reinterpret_cast<const uint4*>(text + at + 16u * j);
        w[4 * j + 0] = v.x;
        w[4 * j + 1] = v.y;
        w[4 * j + 2] = v.z;
        w[4 * j + 3] = v.w;
    }
}

__global__ __launch_bounds__(kFaThreads) void vk_fa_summary_kernel(const uint8_t* base, FaMeta m, uint32_t* ukey) {
    __shared__ uint32_t s_wave[kFaThreads / 64];
    uint64_t u0, u1;
    const uint32_t s = fa_locate(m, blockIdx.x, &u0, &u1);
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    for (uint64_t u = u0; u < u1; ++u) {
        uint32_t w[kFaLaneBytes / 4], n;
        uint64_t c0;
        fa_load(text, len, u, m.unit_bytes, w, &c0, &n);
        const bool first_ls = n && (c0 == 0 || text[c0 - 1] == '\n');
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        uint32_t total;
        (void)fa_block_excl_max(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, s_wave, &total);
        if (threadIdx.x == 0) ukey[m.unit_first[s] + u] = total ? 2u | (total & 1u) : 0u;
    }
}

__global__ __launch_bounds__(kFaThreads) void vk_fa_scan_kernel(const uint8_t* base, FaMeta m, const uint32_t* ukey, uint32_t* carry,
                                                                uint32_t* status) {
    __shared__ uint32_t s_wave[kFaThreads / 64];
    const uint32_t s = blockIdx.x;
    const uint64_t first = m.unit_first[s], nunits = m.unit_first[s + 1] - first;   // (nunits < 2^30: the caller checks)
    uint32_t running = 0;
    for (uint64_t t = 0; t < nunits; t += kFaThreads) {
        const uint64_t u = t + threadIdx.x;
        const uint32_t k = u < nunits ? ukey[first + u] : 0u;
        uint32_t total;
        uint32_t excl = fa_block_excl_max(k ? (static_cast<uint32_t>(u + 1) << 1) | (k & 1u) : 0u, s_wave, &total);
        if (running > excl) excl = running;
        if (u < nunits) carry[first + u] = excl & 1u;   // (nothing before: not in a header line)
        if (total > running) running = total;
    }
    if (threadIdx.x == 0) status[s] = m.lens[s] && base[m.offs[s]] != '>' ? 1u : 0u;   // VK_ST_BAD_START
}

template <int K>
struct FaAdd {
    uint32_t* table;   // LDS (K <= 7) or the sample's row (K = 8, 9)
    __device__ inline void operator()(uint32_t code, uint32_t n) { atomicAdd(table + code, n); }
};

template <int K>
__global__ __launch_bounds__(kFaThreads) void vk_fa_count_kernel(const uint8_t* base, FaMeta m, const uint32_t* carry, uint32_t* hist,
                                                                 unsigned long long* bases) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    constexpr bool LDSH = K <= 7;
    __shared__ uint32_t s_hist[LDSH ? NCODE : 1];
    __shared__ uint32_t s_wave[kFaThreads / 64];
    uint64_t u0, u1;
    const uint32_t s = fa_locate(m, blockIdx.x, &u0, &u1);
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    if (text[0] != '>') return;   // VK_ST_BAD_START (a sample with a workgroup is not empty): its histogram is not used
    uint32_t* row = hist + static_cast<size_t>(s) * NCODE;
    if (LDSH) {
        for (uint32_t i = threadIdx.x; i < NCODE; i += kFaThreads) s_hist[i] = 0;
        __syncthreads();
    }
    FaAdd<K> add{LDSH ? s_hist : row};
    uint32_t my_bases = 0;
    for (uint64_t u = u0; u < u1; ++u) {
        uint32_t w[kFaLaneBytes / 4], n;
        uint64_t c0;
        fa_load(text, len, u, m.unit_bytes, w, &c0, &n);
        const bool first_ls = n && (c0 == 0 || text[c0 - 1] == '\n');
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        uint32_t total;
        const uint32_t excl = fa_block_excl_max(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, s_wave, &total);
        if (n == 0) continue;   // (uniform calls above; nothing below meets a barrier)
        FaWalk wk;
        wk.hdr = excl ? excl & 1u : carry[m.unit_first[s] + u];
        wk.ls = first_ls ? 1u : 0u;
#pragma unroll
        for (uint32_t i = 0; i < kFaLaneBytes; ++i)
            if (i < n) wk.template step<K>(fa_byte(w, i), true, add);
        for (uint64_t p = c0 + n; p < len && wk.template more<K>(); ++p) wk.template step<K>(text[p], false, add);
        wk.flush(add);
        my_bases += wk.bases;
    }
    // the sample's sequence bytes: a sum per wave, one atomic each
    for (uint32_t d = 32; d; d >>= 1) my_bases += __shfl_down(my_bases, d, 64);
    if ((threadIdx.x & 63u) == 0 && my_bases) atomicAdd(bases + s, static_cast<unsigned long long>(my_bases));
    if (LDSH) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < NCODE; i += kFaThreads) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(row + i, v);
        }
    }
}

#endif  // VK_FASTA_LANE_ONLY

}  // namespace

#endif  // VK_FASTA_H
