// vk_dist.h -- `compare`: exact squared Euclidean distances between varKode images and the nearest neighbours of every
// query among the references.  Part of the one translation unit vkimg.hip (device code for gfx950; see the notes there).
//
// The rule ("`compare`: the rule"; tests/dist_ref.py is the same rule in NumPy): queries Q u8 [nq, P],
// references R u8 [nr, P], d2(i, j) = sum_p (Q[i,p] - R[j,p])^2, an exact integer below 2^34; reference j is eligible for
// query i if qg[i] is kDistNoGroup or rg[j] != qg[i]; the neighbours of i are its N eligible references with the
// smallest (d2, j), written in that order, the slots left over filled with kDistNoIdx and kDistNoD2.
//
// Launch sequence of vk_dist_device:
//   vk_dist_prep_kernel    a workgroup per image: pixels centred (s = x - 128, i8), the row padded with 0 to kDistK bytes
//                          (a padded pixel is 128 on both sides and adds nothing), |s|^2 as u64.  Centring cancels in
//                          every difference: d2 = |s|^2 + |t|^2 - 2 s.t needs no correction term.
//   per strip of query rows (dist_strip_rows: what the workspace holds, or VKIMG_DIST_STRIP):
//   vk_dist_tile_kernel    a workgroup per kDistTile x kDistTile tile of the strip: s.t with the i8 matrix cores, d2 written
//                          to the strip [rows][nr] u64 (and to the caller's matrix)
//   vk_dist_select_kernel  a workgroup per row of the strip: the N smallest eligible keys (d2 << bits | j)
//
// The tile kernel.  256 threads = 4 wavefronts in 2 x 2, each owning 64 x 64 of the tile as 2 x 2 accumulators of
// __builtin_amdgcn_mfma_i32_32x32x32_i8 (16 i32 registers each).  Operands go global -> registers -> LDS in steps of
// kDistK = 128 pixels, the next step's loads in flight while this one is multiplied.
//   Lane maps.  The instruction computes D[m][n] += sum_k A[m][k] B[k][n]; a lane holds 16 bytes of A and 16 of B.
//   Lane l (r = l & 31, h = l >> 5) supplies A[row r][k = 16 h + e] and B[k = 16 h + e][col r], e = 0..15 the byte of its
//   fragment; D is laid out as for every other type of this shape: register g of lane l is
//   D[row (g & 3) + 8 (g >> 2) + 4 h][col r].  Here A's rows are queries and B's columns are references, and both
//   fragments are read from the SAME 16 pixels (tile row r, bytes 32 s + 16 h .. + 16 of K sub-step s), so the product
//   is right under any bijection between (h, e) and k that A and B share: only the row/column maps can go wrong, and
//   the asymmetric `structured` case of tests/dist_cases.py (swapped or permuted rows and columns change it) holds them.
//   LDS.  A row of a staged operand is 128 bytes of pixels + 16 of padding = 144: a ds_read_b128 is served in groups of
//   16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32), a group reads 16 different rows at one
//   byte offset, and 144 = 9 x 16 puts row r on 16-byte slot 9 r mod 16 of the 256-byte bank row: 9 is odd and each group's
//   rows cover all 16 residues mod 16 ({0-3, 12-15, 4-11 (from 20-27)}, ...), so a group touches every slot once.  Rows of
//   128 bytes unpadded would put all 16 rows on 2 slots.
//   The slice.  |s.t| reaches 128^2 P = 2^32 at P = 512^2, past an i32.  The accumulators run over at most
//   kDistSlice = 65,536 pixels (|sum| <= 2^30), are folded into the u64 in the strip (dist_fold) and start from zero.
//
// The address, slice and key arithmetic, the prep and the per-row selection (dist_*) compile for the host
// (VK_DIST_HOST_ONLY): tests/emul/dist_emul.cpp runs them against tests/dist_ref.py with the matrix instruction stood in
// by a plain loop.
#ifndef VK_DIST_H
#define VK_DIST_H

#include <cstdint>

// rows of a strip (0: as many as kDistStripBytes hold; the emulation and VKIMG_DIST_STRIP shrink it)
#ifndef VK_DIST_STRIP
#define VK_DIST_STRIP 0
#endif

namespace {

constexpr uint32_t kDistTile = 128;                  // queries and references of a workgroup's tile
constexpr uint32_t kDistK = 128;                     // pixels of a K step = the granule rows are padded to
constexpr uint32_t kDistLdsRow = kDistK + 16;        // bytes of a staged row (see LDS above)
constexpr uint32_t kDistSlice = 65536;               // pixels an i32 accumulator runs over: 128^2 * 65,536 = 2^30
constexpr uint32_t kDistThreads = 256;
constexpr uint32_t kDistSelThreads = 256;
constexpr uint32_t kDistMaxN = 64;
constexpr uint64_t kDistMaxRefs = 1ull << 30, kDistMaxPix = 1ull << 20;
constexpr uint32_t kDistNoGroup = 0xFFFFFFFFu, kDistNoIdx = 0xFFFFFFFFu;
constexpr uint64_t kDistNoD2 = ~0ull, kDistNoKey = ~0ull;
constexpr uint64_t kDistStripBytes = 256ull << 20;   // of the strip in the workspace

static_assert(kDistSlice % kDistK == 0 && 128ull * 128ull * kDistSlice <= (1ull << 30), "a slice's sum fits an i32");
static_assert(512ull * 512ull * 255ull * 255ull < (1ull << 34), "the largest shipped image's d2 and any j share a u64 key");

__host__ __device__ inline uint64_t dist_padded(uint64_t npix) { return (npix + kDistK - 1) / kDistK * kDistK; }

// Query rows of a strip: as many as kDistStripBytes hold (whole tiles, one at least), no more than asked for.
__host__ __device__ inline uint64_t dist_strip_rows(uint64_t nq, uint64_t nr, uint64_t asked) {
    uint64_t rows = kDistStripBytes / (8 * (nr ? nr : 1)) / kDistTile * kDistTile;
    if (rows < kDistTile) rows = kDistTile;
    const uint64_t all = (nq + kDistTile - 1) / kDistTile * kDistTile;
    if (rows > all) rows = all;
    if (asked && asked < rows) rows = asked;
    return rows;
}

// A key is d2 << bits | j: ordering and tie-break are one unsigned compare.  bits: the width of j, 1..30.  Up to
// 264,208 pixels (every shipped mapping) d2 < 2^34 and any nr fits; larger images leave j fewer bits (dist_key_fits).
__host__ __device__ inline uint32_t dist_idx_bits(uint64_t nr) {
    uint32_t b = 1;
    while ((1ull << b) < nr) ++b;
    return b;
}
__host__ __device__ inline bool dist_key_fits(uint64_t npix, uint32_t bits) {   // (every key below kDistNoKey)
    return 255ull * 255ull * npix + 1 < (1ull << (64 - bits));
}
__host__ __device__ inline uint64_t dist_key(uint64_t d2, uint32_t j, uint32_t bits) { return (d2 << bits) | j; }
__host__ __device__ inline uint64_t dist_key_d2(uint64_t key, uint32_t bits) { return key >> bits; }
__host__ __device__ inline uint32_t dist_key_idx(uint64_t key, uint32_t bits) { return static_cast<uint32_t>(key & ((1ull << bits) - 1ull)); }

// A slice's sum folded into the distance so far (which starts as |s|^2 + |t|^2).
__host__ __device__ inline uint64_t dist_fold(uint64_t d2, int32_t dot) {
    return d2 - 2 * static_cast<uint64_t>(static_cast<int64_t>(dot));
}

// Prep, thread t of n: the image's pixels centred into its padded row; returns the thread's share of |s|^2.
__host__ __device__ inline uint64_t dist_prep_lane(const uint8_t* x, int8_t* s, uint64_t npix, uint64_t padded, uint32_t t, uint32_t n) {
    uint64_t sum = 0;
    for (uint64_t p = t; p < padded; p += n) {
        const int32_t v = p < npix ? static_cast<int32_t>(x[p]) - 128 : 0;
        s[p] = static_cast<int8_t>(v);
        sum += static_cast<uint64_t>(v * v);
    }
    return sum;
}

// Selection: the smallest eligible key of the row's entries j = start, start + stride, .. above `after` (any, without
// `have_after`); kDistNoKey if there is none.  Keys are distinct (they hold j), so "above" never skips a tie.
// Thread t of a workgroup owns the entries t, t + kDistSelThreads, ..; when its wavefront looks through them again, lane
// x takes every 64th of them: start t + kDistSelThreads x, stride 64 kDistSelThreads.
__host__ __device__ inline uint64_t dist_lane_min(const uint64_t* row, uint32_t nr, const uint32_t* rgroup, uint32_t qgroup,
                                                  uint32_t bits, uint64_t after, bool have_after, uint32_t start, uint32_t stride) {
    uint64_t best = kDistNoKey;
    for (uint32_t j = start; j < nr; j += stride) {
        if (qgroup != kDistNoGroup && rgroup[j] == qgroup) continue;
        const uint64_t key = dist_key(row[j], j, bits);
        if (have_after && key <= after) continue;
        best = key < best ? key : best;
    }
    return best;
}

// A row's slot `rank`: the key's two halves, or the fill.
__host__ __device__ inline void dist_put(uint64_t key, uint32_t bits, uint32_t* idx, uint64_t* d2) {
    *idx = key == kDistNoKey ? kDistNoIdx : dist_key_idx(key, bits);
    *d2 = key == kDistNoKey ? kDistNoD2 : dist_key_d2(key, bits);
}

#ifndef VK_DIST_HOST_ONLY

typedef int dist_v4i __attribute__((ext_vector_type(4)));
typedef int dist_v16i __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(kDistThreads) vk_dist_prep_kernel(const uint8_t* x, int8_t* s, uint64_t* norms, uint64_t npix,
                                                                   uint64_t padded) {
    __shared__ uint64_t part[kDistThreads / 64];
    const uint64_t img = blockIdx.x;
    uint64_t sum = dist_prep_lane(x + img * npix, s + img * padded, npix, padded, threadIdx.x, kDistThreads);
    for (uint32_t d = 32; d; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t v = 0;
        for (uint32_t w = 0; w < kDistThreads / 64; ++w) v += part[w];
        norms[img] = v;
    }
}

// q, r: prepared rows of `padded` bytes; rows [q0, q0 + rows) of the queries against all nr references; strip [rows][nr].
__global__ void __launch_bounds__(kDistThreads) vk_dist_tile_kernel(const int8_t* __restrict__ q, const int8_t* __restrict__ r,
                                                                   const uint64_t* __restrict__ qnorm, const uint64_t* __restrict__ rnorm,
                                                                   uint64_t q0, uint32_t rows, uint32_t nr, uint32_t jtiles, uint64_t padded,
                                                                   uint64_t* __restrict__ strip, uint64_t* __restrict__ matrix) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_a[kDistTile * kDistLdsRow];
    __shared__ __attribute__((aligned(16))) uint8_t lds_b[kDistTile * kDistLdsRow];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t wm = (wave >> 1) * 64u, wn = (wave & 1u) * 64u;   // the wavefront's corner in the tile
    const uint32_t lr = lane & 31u, lh = lane >> 5;
    // the tile's corner in the strip (a one-dimensional grid, tiles of one row of tiles next to each other: they share queries)
    const uint32_t i0 = blockIdx.x / jtiles * kDistTile, j0 = blockIdx.x % jtiles * kDistTile;
    // staging: a thread moves 16 bytes of 4 rows of each operand per step (row t / 8 + 32 c, bytes 16 (t % 8) ..); rows
    // past the end are read from the last row (never written out)
    const uint32_t srow = t >> 3, sbyte = (t & 7u) * 16u;
    const int8_t* ga[4];
    const int8_t* gb[4];
    for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t ia = min(i0 + srow + 32u * c, rows - 1u), jb = min(j0 + srow + 32u * c, nr - 1u);
        ga[c] = q + (q0 + ia) * padded + sbyte;
        gb[c] = r + static_cast<uint64_t>(jb) * padded + sbyte;
    }
    dist_v4i ra[4], rb[4];
    for (uint64_t k0 = 0; k0 < padded; k0 += kDistSlice) {
        const uint64_t k1 = min(k0 + static_cast<uint64_t>(kDistSlice), padded);
        dist_v16i acc[2][2];
        for (uint32_t m = 0; m < 2; ++m)
            for (uint32_t n = 0; n < 2; ++n)
                for (uint32_t g = 0; g < 16; ++g) acc[m][n][g] = 0;
        for (uint32_t c = 0; c < 4; ++c) {
            ra[c] = *reinterpret_cast<const dist_v4i*>(ga[c] + k0);
            rb[c] = *reinterpret_cast<const dist_v4i*>(gb[c] + k0);
        }
        for (uint64_t k = k0; k < k1; k += kDistK) {
            __syncthreads();   // (the step before has been read)
            for (uint32_t c = 0; c < 4; ++c) {
                *reinterpret_cast<dist_v4i*>(lds_a + (srow + 32u * c) * kDistLdsRow + sbyte) = ra[c];
                *reinterpret_cast<dist_v4i*>(lds_b + (srow + 32u * c) * kDistLdsRow + sbyte) = rb[c];
            }
            __syncthreads();
            if (k + kDistK < k1) {
                for (uint32_t c = 0; c < 4; ++c) {
                    ra[c] = *reinterpret_cast<const dist_v4i*>(ga[c] + k + kDistK);
                    rb[c] = *reinterpret_cast<const dist_v4i*>(gb[c] + k + kDistK);
                }
            }
            for (uint32_t s = 0; s < kDistK / 32; ++s) {
                dist_v4i fa[2], fb[2];
                for (uint32_t m = 0; m < 2; ++m)
                    fa[m] = *reinterpret_cast<const dist_v4i*>(lds_a + (wm + 32u * m + lr) * kDistLdsRow + 32u * s + 16u * lh);
                for (uint32_t n = 0; n < 2; ++n)
                    fb[n] = *reinterpret_cast<const dist_v4i*>(lds_b + (wn + 32u * n + lr) * kDistLdsRow + 32u * s + 16u * lh);
                for (uint32_t m = 0; m < 2; ++m)
                    for (uint32_t n = 0; n < 2; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
            }
        }
        // the slice's sums into the strip: register g of lane (lr, lh) is query row (g & 3) + 8 (g >> 2) + 4 lh, reference lr
        const bool first = k0 == 0, last = k1 == padded;
        for (uint32_t n = 0; n < 2; ++n) {
            const uint32_t j = j0 + wn + 32u * n + lr;
            if (j >= nr) continue;
            const uint64_t rn = rnorm[j];
            for (uint32_t m = 0; m < 2; ++m)
                for (uint32_t g = 0; g < 16; ++g) {
                    const uint32_t i = i0 + wm + 32u * m + (g & 3u) + 8u * (g >> 2) + 4u * lh;
                    if (i >= rows) continue;
                    uint64_t* at = strip + static_cast<uint64_t>(i) * nr + j;
                    const uint64_t v = dist_fold(first ? qnorm[q0 + i] + rn : *at, acc[m][n][g]);
                    *at = v;
                    if (last && matrix) matrix[(q0 + i) * nr + j] = v;
                }
        }
    }
}

__device__ inline uint64_t dist_wave_min(uint64_t v) {   // (every lane gets it)
    for (uint32_t d = 32; d; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// A workgroup per row of the strip.  Every thread holds the smallest key of its entries; the smallest of those is the
// next neighbour, and only the entries of the thread that held it are looked through again -- by its whole wavefront, a
// lane per 64th of them (one thread alone walked them a load behind the other: the first build's selection took as long
// as the tiles).
__global__ void __launch_bounds__(kDistSelThreads) vk_dist_select_kernel(const uint64_t* __restrict__ strip, uint64_t q0, uint32_t nr,
                                                                        const uint32_t* __restrict__ qgroup, const uint32_t* __restrict__ rgroup,
                                                                        uint32_t nn, uint32_t bits, uint32_t* __restrict__ idx, uint64_t* __restrict__ d2) {
    __shared__ uint64_t part[2][kDistSelThreads / 64];
    const uint64_t i = q0 + blockIdx.x;
    const uint64_t* row = strip + static_cast<uint64_t>(blockIdx.x) * nr;
    const uint32_t qg = qgroup ? qgroup[i] : kDistNoGroup;
    const uint32_t t = threadIdx.x;
    uint64_t mine = dist_lane_min(row, nr, rgroup, qg, bits, 0, false, t, kDistSelThreads);
    for (uint32_t rank = 0; rank < nn; ++rank) {
        const uint64_t v = dist_wave_min(mine);
        if ((t & 63u) == 0) part[rank & 1u][t >> 6] = v;
        __syncthreads();   // (part[] alternates: a thread a rank ahead writes the other half)
        uint64_t least = part[rank & 1u][0];
        for (uint32_t w = 1; w < kDistSelThreads / 64; ++w) least = part[rank & 1u][w] < least ? part[rank & 1u][w] : least;
        // (every lane read the same: as a scalar, so that the loop is left by a scalar branch and its shuffles stay convergent)
        const uint64_t best = static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(least)))) |
                              static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(least >> 32)))) << 32;
        if (t == 0) dist_put(best, bits, idx + i * nn + rank, d2 + i * nn + rank);
        if (best == kDistNoKey) {   // (every thread sees the same: the fill)
            for (uint32_t f = rank + 1 + t; f < nn; f += kDistSelThreads) dist_put(kDistNoKey, bits, idx + i * nn + f, d2 + i * nn + f);
            break;
        }
        const unsigned long long held = __ballot(mine == best);   // (keys are distinct: one lane of one wavefront)
        if (held) {
            const uint32_t owner = (t & ~63u) + static_cast<uint32_t>(__builtin_ctzll(held));
            const uint64_t next = dist_wave_min(dist_lane_min(row, nr, rgroup, qg, bits, best, true,
                                                              owner + kDistSelThreads * (t & 63u), kDistSelThreads * 64u));
            if (t == owner) mine = next;
        }
    }
}

#endif  // VK_DIST_HOST_ONLY

}  // namespace

#endif  // VK_DIST_H
