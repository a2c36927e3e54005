// vk_sketch.h -- `image / query --spectrum-sketch` and `distance`: a bottom-s MinHash sketch taken from a sample's
// spectrum table while it lies in HBM, and the comparison of every pair of sketches.  Part of the one translation unit
// vkimg.hip (device code for gfx950; see the notes there).
//
// The rule ("`--spectrum-sketch` and `distance`: the rule"; tests/sketch_ref.py is the same rule in
// Python, twice): a held slot (its key is not all ones) is ELIGIBLE when its count is at least min_count; a sample's
// sketch is the min(s, eligible) smallest sc_mix(key) over its eligible slots, ascending, the rest of its row all ones.
// A pair of sketches: seen = min(s, |Sa u Sb|), shared = the values among the seen smallest of Sa u Sb that lie in both.
//
// Launch sequence of vk_sketch_device (after vk_spectrum_device; nothing here allocates or synchronises, so what the
// device decides -- how many rounds a sample needs -- is a fixed sequence whose later workgroups read SkState::round
// and return):
//   vk_sk_hist_kernel x 6   round r: workgroups over a sample's slots count, in 2,048 LDS bins flushed once, digit r (11
//   vk_sk_pick_kernel x 6   bits, the last 9) of the eligible hashes under the prefix so far; one workgroup per sample
//                           finds the bin where the cumulative count crosses s and extends the prefix.  Selection ends
//                           as soon as the hashes below the prefix and those of the crossing bin fit the sample's
//                           candidate buffer (s + slack): for spread hashes in round 0, at once when eligible <= capacity
//   vk_sk_compact_kernel    one more pass: every candidate hash to the buffer -- gathered in LDS with one LDS atomic per
//                           wave, flushed behind one cursor atomic per 2,048 and more candidates of a workgroup
//   vk_sk_run_kernel        bitonic sort of runs of 2,048 candidates in LDS
//   vk_sk_merge_kernel x L  merge-path merges of neighbouring runs in global memory, ping-pong; L is fixed by the largest
//                           buffer of the call, a level past a sample's candidates copies
//   vk_sk_finish_kernel     the first `length` candidates to the row, eligible and length to d_info
// vk_sketch_pairs_device is vk_sk_pairs_kernel alone: a wavefront per pair cuts the two-list merge into 64 diagonals.
// vk_sketch_pair_blocks_device is vk_sk_pair_blocks_kernel alone: the same pair, its counts split by the block h & 63 of
// each value (`tree --replicates`: the delete-half jackknife sums the blocks it keeps).
//
// The lane-local code (sk_eligible, sk_under, sk_digit, sk_candidate, sk_diag, sk_walk, sk_walk_blocks, sk_merge) compiles for the host:
// tests/emul/sketch_emul.cpp runs it, a lane at a time, against tests/sketch_ref.py.
#ifndef VK_SKETCH_H
#define VK_SKETCH_H

#include <cstdint>

#include "vk_spectrum.h"

namespace {

constexpr uint32_t kSkMinS = 64, kSkMaxS = 1u << 20;        // VK_SKETCH_MIN, VK_SKETCH_MAX (vkimg.h)
constexpr uint32_t kSkDigitBits = 11, kSkBins = 1u << kSkDigitBits;
constexpr uint32_t kSkRounds = 6;                            // 5 digits of 11 bits and one of 9
constexpr uint32_t kSkDone = kSkRounds;                      // SkState::round when the selection has ended
constexpr uint32_t kSkRun = 2048;                            // hashes of an LDS-sorted run, and outputs of a merge workgroup
constexpr uint32_t kSkMergePerLane = 8;                      // outputs a lane merges: a workgroup's are a run
constexpr uint64_t kSkMinSlack = 4096;                       // a candidate buffer holds s + max(this, nslots / 2,048) hashes
constexpr uint64_t kSkMaxSlots = 1ull << 31;                 // (a bin is 32-bit)
constexpr uint64_t kSkMinPerBlock = kSpSlotsPerBlock;        // slots per workgroup of the table passes: this, or nslots / 1,024 if more
constexpr uint64_t kSkMaxBlocksPerSample = 1024;
constexpr uint32_t kSkAll = 0, kSkUpTo = 1, kSkStrict = 2;   // SkState::mode
constexpr uint64_t kSkMaxSide = 1ull << 20, kSkMaxPairs = 1ull << 32;
constexpr uint32_t kSkBlocks = 64;                           // jackknife blocks: a value h lies in block h & 63
constexpr uint64_t kSkMaxBlockPairs = 1ull << 26;            // pairs of a vk_sketch_pair_blocks_device call

__device__ inline bool sk_eligible(uint64_t key, uint32_t count, uint32_t min_count) { return key != kScEmpty && count >= min_count; }

// round r's digit lies at these bits of a hash
__device__ inline uint32_t sk_shift(uint32_t round) { return round + 1u < kSkRounds ? 64u - kSkDigitBits * (round + 1u) : 0u; }
__device__ inline uint32_t sk_bits(uint32_t round) { return round + 1u < kSkRounds ? kSkDigitBits : 64u - kSkDigitBits * (kSkRounds - 1u); }
__device__ inline uint32_t sk_digit(uint64_t h, uint32_t round) { return static_cast<uint32_t>(h >> sk_shift(round)) & ((1u << sk_bits(round)) - 1u); }
// does the hash begin with the digits of the rounds before this one?
__device__ inline bool sk_under(uint64_t h, uint64_t prefix, uint32_t round) { return round == 0u || (h >> (64u - kSkDigitBits * round)) == prefix; }
// is the hash a candidate under the selection's last word?
__device__ inline bool sk_candidate(uint64_t h, uint32_t mode, uint32_t shift, uint64_t prefix) {
    return mode == kSkAll || (mode == kSkUpTo ? (h >> shift) <= prefix : (h >> shift) < prefix);
}

// Merge path: of the first d values of the merge of A[0 .. la) and B[0 .. lb) (both ascending; of equal values A's
// comes first), how many are A's?  d <= la + lb.  Reads A[i] only for i < la and B[j] only for j < lb.
__device__ inline uint32_t sk_diag(const uint64_t* A, uint32_t la, const uint64_t* B, uint32_t lb, uint32_t d) {
    uint32_t lo = d > lb ? d - lb : 0u, hi = d < la ? d : la;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (A[mid] <= B[d - 1u - mid]) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// `steps` values of the merge from (i, j) on; A and B strictly ascending.  A value of B that equals the A before it is
// a DUPLICATE (its partner may lie in the segment before: A[i - 1] is read wherever it lies); every other value is a
// distinct value of the union.  A duplicate counts while the distinct values up to it, base included, are at most limit.
__device__ inline void sk_walk(const uint64_t* A, uint32_t la, const uint64_t* B, uint32_t lb, uint32_t i, uint32_t j, uint32_t steps,
                               uint64_t base, uint64_t limit, uint32_t* distinct, uint32_t* dups) {
    uint32_t nd = 0, du = 0;
    for (uint32_t t = 0; t < steps; ++t) {
        if (j >= lb || (i < la && A[i] <= B[j])) {
            ++i;
            ++nd;
        } else {
            if (i > 0u && A[i - 1u] == B[j]) du += base + nd <= limit ? 1u : 0u;
            else ++nd;
            ++j;
        }
    }
    *distinct = nd;
    *dups = du;
}

// The walk once more, for the per-block counts of the jackknife (block of a value h: h & 63): every distinct value whose
// ordinal -- base and the distinct values up to it, itself included -- is at most limit goes to seen(h), every duplicate
// that sk_walk would count to shared(h).
template <class Seen, class Shared>
__device__ inline void sk_walk_blocks(const uint64_t* A, uint32_t la, const uint64_t* B, uint32_t lb, uint32_t i, uint32_t j,
                                      uint32_t steps, uint64_t base, uint64_t limit, Seen seen, Shared shared) {
    uint32_t nd = 0;
    for (uint32_t t = 0; t < steps; ++t) {
        if (j >= lb || (i < la && A[i] <= B[j])) {
            ++nd;
            if (base + nd <= limit) seen(A[i]);
            ++i;
        } else {
            if (i > 0u && A[i - 1u] == B[j]) {
                if (base + nd <= limit) shared(B[j]);
            } else {
                ++nd;
                if (base + nd <= limit) seen(B[j]);
            }
            ++j;
        }
    }
}

// n values of the merge from (i, j) on to out (n <= la - i + lb - j)
__device__ inline void sk_merge(const uint64_t* A, uint32_t la, const uint64_t* B, uint32_t lb, uint32_t i, uint32_t j, uint32_t n,
                                uint64_t* out) {
    for (uint32_t t = 0; t < n; ++t) out[t] = j >= lb || (i < la && A[i] <= B[j]) ? A[i++] : B[j++];
}

#ifndef VK_SKETCH_LANE_ONLY

static_assert(kSkMergePerLane * kClThreads == kSkRun, "a merge workgroup writes a run");
constexpr uint32_t kSkPairsPerBlock = kClThreads / 64;
constexpr uint32_t kSkTile = 2048;   // slots between two looks at the compaction's LDS buffer, which holds twice as many hashes

struct SkState {          // a sample's selection
    uint64_t prefix;      // the crossing bins' digits so far
    uint64_t below;       // eligible hashes below the prefix
    uint64_t eligible;
    uint64_t cand_base;   // the sample's first candidate in the two buffers
    uint64_t per_block;   // slots of a workgroup of the table passes
    uint32_t round;       // the round that runs next; kSkDone when the selection has ended
    uint32_t mode, shift; // a candidate: sk_candidate(hash, mode, shift, prefix)
    uint32_t cursor;      // candidates the compaction met
    uint32_t cap;         // hashes the sample's buffer holds (a multiple of kSkRun)
    uint32_t pad;
};

__device__ inline uint32_t sk_ncand(const SkState& S) { return S.cursor < S.cap ? S.cursor : S.cap; }

// the workgroup's sample and its slots [first, end)
__device__ inline uint32_t sk_locate(const uint64_t* block_base, uint32_t nsamples, const SkState* st, const uint64_t* nslots,
                                     uint64_t* first, uint64_t* end) {
    const uint32_t si = cl_find_u64(block_base, nsamples, blockIdx.x);
    const uint64_t per = st[si].per_block, n = nslots[si];
    *first = (blockIdx.x - block_base[si]) * per;
    *end = *first + per < n ? *first + per : n;
    return si;
}

__global__ void __launch_bounds__(kClThreads) vk_sk_hist_kernel(const uint64_t* block_base, uint32_t nsamples, const uint64_t* slot_base,
                                                               const uint64_t* nslots, const uint64_t* keys, const uint32_t* counts,
                                                               const uint32_t* status, uint32_t min_count, uint32_t round,
                                                               const SkState* st, uint32_t* hist) {
    __shared__ uint32_t s_bins[kSkBins];
    uint64_t first, end;
    const uint32_t si = sk_locate(block_base, nsamples, st, nslots, &first, &end);
    if (status[si] != 0 || st[si].round != round) return;   // (uniform: the whole workgroup)
    const uint64_t prefix = st[si].prefix;
    for (uint32_t b = threadIdx.x; b < kSkBins; b += kClThreads) s_bins[b] = 0;
    __syncthreads();
    const uint64_t* k = keys + slot_base[si];
    const uint32_t* c = counts + slot_base[si];
    for (uint64_t i = first + threadIdx.x; i < end; i += kClThreads) {
        const uint64_t key = k[i];
        if (!sk_eligible(key, c[i], min_count)) continue;
        const uint64_t h = sc_mix(key);
        if (sk_under(h, prefix, round)) atomicAdd(&s_bins[sk_digit(h, round)], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSkBins; b += kClThreads) {
        const uint32_t v = s_bins[b];
        if (v) atomicAdd(hist + static_cast<uint64_t>(kSkBins) * si + b, v);
    }
}

// One workgroup per sample: the bin where the cumulative count crosses what is still needed.  Leaves the bins zero.
__global__ void __launch_bounds__(kClThreads) vk_sk_pick_kernel(const uint32_t* status, uint32_t round, uint32_t s, SkState* st,
                                                               uint32_t* hist) {
    __shared__ uint64_t sh[kClThreads];
    const uint32_t si = blockIdx.x;
    SkState* S = st + si;
    if (status[si] != 0 || S->round != round) return;
    const uint64_t prefix0 = S->prefix, below0 = S->below, cap = S->cap;
    uint32_t* h = hist + static_cast<uint64_t>(kSkBins) * si;
    constexpr uint32_t kPer = kSkBins / kClThreads;
    uint32_t v[kPer];
    uint64_t sum = 0;
    for (uint32_t j = 0; j < kPer; ++j) {
        v[j] = h[threadIdx.x * kPer + j];
        h[threadIdx.x * kPer + j] = 0;
        sum += v[j];
    }
    sh[threadIdx.x] = sum;
    __syncthreads();   // (every lane has read the state)
    for (uint32_t d = 1; d < kClThreads; d <<= 1) {
        const uint64_t t = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    const uint64_t incl = sh[threadIdx.x], excl = incl - sum, total = sh[kClThreads - 1];
    if (round == 0) {
        if (threadIdx.x == 0) S->eligible = total;
        if (total <= cap) {   // every eligible hash is a candidate
            if (threadIdx.x == 0) {
                S->mode = kSkAll;
                S->round = kSkDone;
            }
            return;
        }
    }
    const uint64_t need = s - below0;   // (1 at least, and at most this round's total)
    if (excl < need && need <= incl) {  // one lane
        uint64_t cum = excl;
        uint32_t j = 0;
        while (j + 1 < kPer && cum + v[j] < need) cum += v[j++];
        const uint64_t below = below0 + cum;
        const bool done = below + v[j] <= cap, last = round + 1 == kSkRounds;
        S->prefix = (prefix0 << sk_bits(round)) | (threadIdx.x * kPer + j);
        S->below = below;
        S->shift = sk_shift(round);
        // (the last round's bin is one value: if even that overflows, equal keys lie in several slots -- the hashes
        // strictly below are then fewer than s, and vk_sk_finish_kernel fills the row with the value itself)
        S->mode = done || !last ? kSkUpTo : kSkStrict;
        S->round = done || last ? kSkDone : round + 1;
    }
}

__global__ void __launch_bounds__(kClThreads) vk_sk_compact_kernel(const uint64_t* block_base, uint32_t nsamples,
                                                                  const uint64_t* slot_base, const uint64_t* nslots,
                                                                  const uint64_t* keys, const uint32_t* counts, const uint32_t* status,
                                                                  uint32_t min_count, SkState* st, uint64_t* cand) {
    uint64_t first, end;
    const uint32_t si = sk_locate(block_base, nsamples, st, nslots, &first, &end);
    if (status[si] != 0) return;   // (uniform: the whole workgroup)
    SkState* S = st + si;
    const uint32_t mode = S->mode, shift = S->shift, cap = S->cap, lane = threadIdx.x & 63u;
    const uint64_t prefix = S->prefix;
    const uint64_t* k = keys + slot_base[si];
    const uint32_t* c = counts + slot_base[si];
    uint64_t* out = cand + S->cand_base;
    // The candidates gather in LDS -- a wave's take their places there with one LDS atomic -- and leave for the sample's
    // buffer behind ONE global atomic, when a further tile might not fit and at the end.  (A global atomic per wave was
    // measured first: at s = 2^20 the million candidates of a 2^30-slot table lie one to a wave instruction, and a
    // million adds to one address made a 3.2 ms pass take 12.9 ms.)
    __shared__ uint64_t s_buf[2 * kSkTile];
    __shared__ uint32_t s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint64_t t0 = first; t0 < end; t0 += kSkTile) {   // (the trip counts are the workgroup's: every lane meets the ballots and barriers)
        for (uint32_t j = 0; j < kSkTile; j += kClThreads) {
            const uint64_t i = t0 + j + threadIdx.x;
            uint64_t hsh = 0;
            bool take = false;
            if (i < end) {
                const uint64_t key = k[i];
                if (sk_eligible(key, c[i], min_count)) {
                    hsh = sc_mix(key);
                    take = sk_candidate(hsh, mode, shift, prefix);
                }
            }
            const uint64_t T = __ballot(take);
            if (T == 0) continue;
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&s_n, static_cast<uint32_t>(__popcll(T)));
            at = sc_uniform(at) + static_cast<uint32_t>(__popcll(T & ((1ull << lane) - 1ull)));
            if (take) s_buf[at] = hsh;   // (at most kSkTile held before the tile, at most kSkTile of the tile)
        }
        __syncthreads();
        const uint32_t n = s_n;
        __syncthreads();   // (every lane has read n before a wave of the next tile adds to it)
        if (n <= kSkTile && t0 + kSkTile < end) continue;   // (the workgroup's: room for another tile, and one follows)
        if (n == 0) continue;
        if (threadIdx.x == 0) {
            s_base = atomicAdd(&S->cursor, n);
            s_n = 0;
        }
        __syncthreads();
        const uint32_t base = s_base;
        // (the selection keeps the candidates within cap: the bound is for a table it was not made for)
        for (uint32_t j = threadIdx.x; j < n; j += kClThreads)
            if (base + j < cap) out[base + j] = s_buf[j];
        __syncthreads();   // (the buffer is read before the next tile writes it)
    }
}

// the workgroup's sample and its chunk of kSkRun candidates (per_sample chunks a sample)
__device__ inline uint32_t sk_chunk(uint32_t per_sample, uint32_t* chunk) {
    *chunk = blockIdx.x % per_sample;
    return blockIdx.x / per_sample;
}

__global__ void __launch_bounds__(kClThreads) vk_sk_run_kernel(const uint32_t* status, const SkState* st, uint32_t per_sample,
                                                              uint64_t* cand) {
    __shared__ uint64_t sh[kSkRun];
    uint32_t chunk;
    const uint32_t si = sk_chunk(per_sample, &chunk);
    if (status[si] != 0) return;
    const uint32_t n = sk_ncand(st[si]);
    const uint64_t r0 = static_cast<uint64_t>(chunk) * kSkRun;
    if (r0 >= n) return;   // (uniform; a run that begins within the candidates lies within the buffer: cap is a multiple of kSkRun)
    uint64_t* run = cand + st[si].cand_base + r0;
    for (uint32_t t = threadIdx.x; t < kSkRun; t += kClThreads) sh[t] = r0 + t < n ? run[t] : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= kSkRun; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < kSkRun / 2; t += kClThreads) {
                const uint32_t lo = 2u * t - (t & (j - 1u)), hi = lo + j;
                const uint64_t a = sh[lo], b = sh[hi];
                if ((a > b) == ((lo & k) == 0u)) {
                    sh[lo] = b;
                    sh[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t t = threadIdx.x; t < kSkRun; t += kClThreads) run[t] = sh[t];
}

// A level: runs of `width` (a multiple of kSkRun) of src merged in pairs into dst.
__global__ void __launch_bounds__(kClThreads) vk_sk_merge_kernel(const uint32_t* status, const SkState* st, uint32_t per_sample,
                                                                uint32_t width, const uint64_t* src, uint64_t* dst) {
    uint32_t chunk;
    const uint32_t si = sk_chunk(per_sample, &chunk);
    if (status[si] != 0) return;
    const uint32_t n = sk_ncand(st[si]);
    const uint32_t npad = (n + kSkRun - 1u) / kSkRun * kSkRun;   // (at most cap)
    if (static_cast<uint64_t>(chunk) * kSkRun >= npad) return;
    const uint32_t o0 = chunk * kSkRun + threadIdx.x * kSkMergePerLane;   // (below npad, with its kSkMergePerLane values)
    const uint32_t a0 = o0 / (2u * width) * (2u * width);              // (npad < 2^31: no overflow)
    const uint32_t la = npad - a0 < width ? npad - a0 : width;
    const uint32_t lb = npad - a0 - la < width ? npad - a0 - la : width;
    const uint64_t* A = src + st[si].cand_base + a0;
    const uint64_t* B = A + la;
    const uint32_t d = o0 - a0, i = sk_diag(A, la, B, lb, d);
    uint64_t v[kSkMergePerLane];
    sk_merge(A, la, B, lb, i, d - i, kSkMergePerLane, v);
    uint64_t* out = dst + st[si].cand_base + o0;
    for (uint32_t t = 0; t < kSkMergePerLane; ++t) out[t] = v[t];
}

__global__ void __launch_bounds__(kClThreads) vk_sk_finish_kernel(const uint32_t* status, const SkState* st, uint32_t per_sample,
                                                                 uint32_t s, const uint64_t* sorted, uint64_t* hashes, uint64_t* info) {
    const uint32_t si = blockIdx.x / per_sample;
    const uint32_t i = (blockIdx.x % per_sample) * kClThreads + threadIdx.x;
    const bool bad = status[si] != 0;
    const SkState S = st[si];
    const uint64_t eligible = bad ? 0 : S.eligible, length = eligible < s ? eligible : s;
    if (i == 0) {
        info[2ull * si] = eligible;
        info[2ull * si + 1] = length;
    }
    if (i >= s) return;
    uint64_t v = ~0ull;
    if (i < length) v = i < sk_ncand(S) ? sorted[S.cand_base + i] : S.prefix;   // (kSkStrict: see vk_sk_pick_kernel)
    hashes[static_cast<uint64_t>(s) * si + i] = v;
}

// A wavefront per pair: the merge of the two sketches, where a common value appears twice, cut into 64 diagonals.
__global__ void __launch_bounds__(kClThreads) vk_sk_pairs_kernel(const uint64_t* q, const uint64_t* qlen, uint32_t nq, const uint64_t* r,
                                                                const uint64_t* rlen, uint32_t nr, uint32_t s, uint32_t* shared,
                                                                uint32_t* seen) {
    const uint32_t wave = sc_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint64_t pair = static_cast<uint64_t>(blockIdx.x) * kSkPairsPerBlock + wave;
    if (pair >= static_cast<uint64_t>(nq) * nr) return;   // (the wave's; no barrier below)
    const uint32_t qi = sc_uniform(static_cast<uint32_t>(pair / nr)), ri = sc_uniform(static_cast<uint32_t>(pair % nr));
    const uint64_t qn = qlen[qi], rn = rlen[ri];
    const uint32_t la = sc_uniform(static_cast<uint32_t>(qn < s ? qn : s)), lb = sc_uniform(static_cast<uint32_t>(rn < s ? rn : s));
    const uint64_t* A = q + static_cast<uint64_t>(s) * qi;
    const uint64_t* B = r + static_cast<uint64_t>(s) * ri;
    const uint32_t n = la + lb, seg = (n + 63u) / 64u;
    const uint32_t d0 = min(lane * seg, n), d1 = min(d0 + seg, n);
    const uint32_t i0 = sk_diag(A, la, B, lb, d0);
    uint32_t distinct, dups;
    sk_walk(A, la, B, lb, i0, d0 - i0, d1 - d0, 0, ~0ull, &distinct, &dups);
    uint32_t incl = distinct;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    const uint32_t all = sc_uniform(static_cast<uint32_t>(__shfl(incl, 63, 64)));
    const uint32_t sn = all < s ? all : s, excl = incl - distinct;
    // the lane where the count crosses `seen` walks again, to the exact stop
    uint32_t mine = incl <= sn ? dups : 0u;
    if (excl <= sn && sn < incl) sk_walk(A, la, B, lb, i0, d0 - i0, d1 - d0, excl, sn, &distinct, &mine);
    for (uint32_t d = 32; d; d >>= 1) mine += __shfl_down(mine, d, 64);
    if (lane == 0) {
        shared[pair] = mine;
        seen[pair] = sn;
    }
}

// vk_sk_pairs_kernel's pair, counted per block: the same diagonals, scan and stop; then every lane whose segment begins at
// or before the stop walks it again and adds into its wave's 2 x 64 counters in LDS.  Lane b writes block b.
__global__ void __launch_bounds__(kClThreads) vk_sk_pair_blocks_kernel(const uint64_t* q, const uint64_t* qlen, uint32_t nq,
                                                                      const uint64_t* r, const uint64_t* rlen, uint32_t nr, uint32_t s,
                                                                      uint32_t* shared, uint32_t* seen) {
    __shared__ uint32_t s_ctr[kSkPairsPerBlock][2][kSkBlocks];
    const uint32_t wave = sc_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint64_t pair = static_cast<uint64_t>(blockIdx.x) * kSkPairsPerBlock + wave;
    const bool valid = pair < static_cast<uint64_t>(nq) * nr;   // (the wave's)
    s_ctr[wave][0][lane] = 0;
    s_ctr[wave][1][lane] = 0;
    __syncthreads();
    if (valid) {
        const uint32_t qi = sc_uniform(static_cast<uint32_t>(pair / nr)), ri = sc_uniform(static_cast<uint32_t>(pair % nr));
        const uint64_t qn = qlen[qi], rn = rlen[ri];
        const uint32_t la = sc_uniform(static_cast<uint32_t>(qn < s ? qn : s)), lb = sc_uniform(static_cast<uint32_t>(rn < s ? rn : s));
        const uint64_t* A = q + static_cast<uint64_t>(s) * qi;
        const uint64_t* B = r + static_cast<uint64_t>(s) * ri;
        const uint32_t n = la + lb, seg = (n + 63u) / 64u;
        const uint32_t d0 = min(lane * seg, n), d1 = min(d0 + seg, n);
        const uint32_t i0 = sk_diag(A, la, B, lb, d0);
        uint32_t distinct, dups;
        sk_walk(A, la, B, lb, i0, d0 - i0, d1 - d0, 0, ~0ull, &distinct, &dups);
        uint32_t incl = distinct;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        const uint32_t all = sc_uniform(static_cast<uint32_t>(__shfl(incl, 63, 64)));
        const uint32_t sn = all < s ? all : s, excl = incl - distinct;
        uint32_t* c_shared = s_ctr[wave][0];
        uint32_t* c_seen = s_ctr[wave][1];
        if (excl <= sn)
            sk_walk_blocks(A, la, B, lb, i0, d0 - i0, d1 - d0, excl, sn,
                           [c_seen](uint64_t h) { atomicAdd(c_seen + (h & (kSkBlocks - 1u)), 1u); },
                           [c_shared](uint64_t h) { atomicAdd(c_shared + (h & (kSkBlocks - 1u)), 1u); });
    }
    __syncthreads();
    if (valid) {
        shared[pair * kSkBlocks + lane] = s_ctr[wave][0][lane];
        seen[pair * kSkBlocks + lane] = s_ctr[wave][1][lane];
    }
}

#endif  // VK_SKETCH_LANE_ONLY

}  // namespace

#endif  // VK_SKETCH_H
