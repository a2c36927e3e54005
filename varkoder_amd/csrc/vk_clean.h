// vk_clean.h -- step B of `varKoder image` (clean_reads, commands/image.py:317-575): raw FASTQ in HBM ->
// deduplicated, trimmed, poly-G trimmed, adapter-trimmed and merged FASTQ text in HBM.
// Part of the one translation unit vkimg.hip (device code for gfx950; see the notes there).
//
// The cleaning rules are this project's restatement of the fastp options the reference passes (INTEGRATION.md,
// "Step B"); tests/clean_ref.py is the same contract in Python and the GPU output must equal it byte for byte.
//
// Launch sequence of vk_clean_device (every kernel lane- or wave-per-item, no grid-wide barrier inside one):
//   vk_cl_init_kernel        per sample: status word from the host's checks (ragged pairs), stats zeroed;
//                            per file: the header start of its first budgeted record
//   vk_cl_nl_count_kernel    per 16 KiB chunk of every file: newlines
//   vk_cl_scan_*             exclusive scan of the chunks' newline counts (hand-written, three phases)
//   vk_cl_nl_write_kernel    per chunk again: every budgeted line end goes to its record (line i of a file is line
//                            i % 4 of record i / 4: `wc -l` / islice(4 n) framing, commands/image.py:117-160, 223-262)
//   vk_cl_hash_kernel        per unit (a pair, or a single-end read): framing check, 64-bit hash of the sequence bytes
//   vk_cl_dedup_kernel       per unit: open addressing; the slot's representative is compared byte for byte, so a
//                            hash collision probes on and never merges distinct reads; the first record of a class
//                            is the atomic min of the ordinals that reached its slot
//   vk_cl_clean_kernel       per unit (lane per pair): trim, poly-G, overlap (2-bit codes, xor / popcount), adapter
//                            trim, merge -> a plan and the unit's output bytes
//   vk_cl_scan_*             exclusive scan of the output bytes
//   vk_cl_write_kernel       wave per unit: the records, byte-coalesced; per-cycle base counts in LDS, one global
//                            add per workgroup
//   vk_cl_finish_kernel      per sample: output length, zero padding to the 16-byte rounded end
#ifndef VK_CLEAN_H
#define VK_CLEAN_H

// VK_TEXT_STRUCTS_ONLY: the constants and plain structs alone, for a host compiler (vk_textplan.h sizes workspaces with them).
#ifndef VK_TEXT_STRUCTS_ONLY
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

namespace {

constexpr uint32_t kClThreads = 256;
constexpr uint32_t kClChunk = 16384;                 // bytes per workgroup of the newline passes: 64 per lane
constexpr uint32_t kClScanItems = 16;                // items per lane of a scan block
constexpr uint32_t kClScanBlock = kClThreads * kClScanItems;
constexpr uint32_t kClUnitsPerBlock = 64;            // units per workgroup of the write kernel (16 per wavefront)
constexpr uint32_t kClEmpty = 0xFFFFFFFFu;
constexpr uint32_t kClCycles = 40;                   // base-frequency cycles (get_basefrequency_sd reads 5..39)
constexpr uint32_t kClOverlapReq = 30;               // fastp's overlap_len_require
constexpr uint32_t kClOverlapCmp = 50;               // positions counted of an offset (fastp's early stop ends at 50)

struct ClFile {          // a file of the launch, in the library's order (by sample, then R1, R2, unpaired)
    uint64_t off, len;   // text in d_text
    uint64_t nrec;       // budgeted records
    uint64_t rec0;       // global index of its first record
    uint64_t chunk0;     // its first chunk
};

struct ClSample {
    uint64_t r1, r2, se;     // global index of the first record of each group
    uint64_t npairs, nse;
    uint64_t out_off, out_cap;
    uint32_t flags;          // VK_CL_* status bits known on the host (ragged pairs)
    uint32_t pad;
};

struct ClRec {           // line ends of a record (~0: not seen); the header starts at h
    uint64_t h, he, se, pe, qe;
};

struct ClPlan {          // what a unit writes
    uint32_t a1, l1, a2, l2;   // R1 / R2 kept as [a, a + l) of the sequence line
    uint32_t m1, t0, m2;       // merged: R1[a1 .. a1 + m1) + rc(R2 kept)[t0 .. t0 + m2)
    uint32_t flags;            // 1 R1 (or the merged read) written, 2 R2 written, 4 merged
};

#ifndef VK_TEXT_STRUCTS_ONLY

// ------------------------------------------------------------------ helpers --

__device__ inline uint32_t cl_nl_in(uint32_t w) {   // newline bytes of a word (exact per byte)
    const uint32_t x = w ^ 0x0A0A0A0Au;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    return t;   // 0x80 in every byte that was '\n'
}

__device__ inline uint32_t cl_find_u64(const uint64_t* base, uint32_t n, uint64_t v) {
    // largest i < n with base[i] <= v (base ascending, base[0] <= v)
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ inline uint8_t cl_comp(uint8_t b) {   // fastp's complement: ACGT / acgt -> upper-case complement, else 'N'
    switch (b | 0x20) {
        case 'a': return 'T';
        case 't': return 'A';
        case 'c': return 'G';
        case 'g': return 'C';
        default: return 'N';
    }
}

__device__ inline bool cl_acgt(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }

// 50 positions of a sequence as 2-bit codes (A0 C1 T2 G3: (b >> 1) & 3, so a complement is code ^ 2) at the even
// bits of lo (positions 0..31) and hi (32..49); n: the non-ACGT flag at the same bit; x: non-ACGT and not 'N'
struct ClWin {
    uint64_t lo, hi, nlo, nhi, xlo, xhi;
};

__device__ inline void cl_push(ClWin& w, uint8_t b) {   // drop position 0, append b at position 49
    const uint64_t c = (b >> 1) & 3u, bad = cl_acgt(b) ? 0u : 1u, ex = (bad && b != 'N') ? 1u : 0u;
    w.lo = (w.lo >> 2) | (w.hi << 62);
    w.hi = (w.hi >> 2) | (c << 34);
    w.nlo = (w.nlo >> 2) | (w.nhi << 62);
    w.nhi = (w.nhi >> 2) | (bad << 34);
    w.xlo = (w.xlo >> 2) | (w.xhi << 62);
    w.xhi = (w.xhi >> 2) | (ex << 34);
}

__device__ inline void cl_push_none(ClWin& w) {          // past the end: a position that is never counted
    w.lo = (w.lo >> 2) | (w.hi << 62);
    w.hi >>= 2;
    w.nlo = (w.nlo >> 2) | (w.nhi << 62);
    w.nhi >>= 2;
    w.xlo = (w.xlo >> 2) | (w.xhi << 62);
    w.xhi >>= 2;
}

// mismatches among the first n (<= 50) positions of two windows, bytes compared as they are: two ACGT codes by
// xor; an ACGT byte against a non-ACGT one always differs; two non-ACGT bytes -- the second window is a reverse
// complement, whose only non-ACGT byte is 'N' -- differ unless the first is 'N' too
__device__ inline uint32_t cl_mism(const ClWin& a, const ClWin& b, uint32_t n) {
    constexpr uint64_t kEven = 0x5555555555555555ull;
    const uint64_t vlo = n >= 32 ? kEven : (((1ull << (2 * n)) - 1) & kEven);
    const uint64_t vhi = n > 32 ? (((1ull << (2 * (n - 32))) - 1) & kEven) : 0ull;
    const uint64_t xl = a.lo ^ b.lo, xh = a.hi ^ b.hi;
    const uint64_t ml = (xl | (xl >> 1)) & kEven, mh = (xh | (xh >> 1)) & kEven;
    const uint64_t nl = a.nlo | b.nlo, nh = a.nhi | b.nhi;
    const uint64_t bl = a.nlo & b.nlo, bh = a.nhi & b.nhi;
    return __popcll(ml & ~nl & vlo) + __popcll(mh & ~nh & vhi) + __popcll((a.nlo ^ b.nlo) & vlo) +
           __popcll((a.nhi ^ b.nhi) & vhi) + __popcll(bl & (a.xlo | b.xlo) & vlo) + __popcll(bh & (a.xhi | b.xhi) & vhi);
}

// s1 = R1 kept (p1[0 .. len1)), s2 = reverse complement of R2 kept (p2[0 .. len2)); fastp 0.23's
// OverlapAnalysis::analyze in closed form: the first offset accepted, forward before backward
__device__ inline bool cl_overlap(const uint8_t* p1, uint32_t len1, const uint8_t* p2, uint32_t len2, int* off_out,
                                  uint32_t* ol_out) {
    ClWin w1 = {}, w2 = {};
    for (uint32_t i = 0; i < kClOverlapCmp; ++i) {
        if (i < len1) cl_push(w1, p1[i]); else cl_push_none(w1);
        if (i < len2) cl_push(w2, cl_comp(p2[len2 - 1 - i])); else cl_push_none(w2);
    }
    const ClWin w1_0 = w1, w2_0 = w2;
    // forward: s1[off + i] against s2[i]
    for (uint32_t off = 0; off + kClOverlapReq < len1; ++off) {
        const uint32_t ol = min(len1 - off, len2), n = min(kClOverlapCmp, ol), lim = min(5u, ol / 5);
        if (cl_mism(w1, w2_0, n) <= lim) {
            *off_out = static_cast<int>(off);
            *ol_out = ol;
            return true;
        }
        const uint32_t j = off + kClOverlapCmp;
        if (j < len1) cl_push(w1, p1[j]); else cl_push_none(w1);
    }
    // backward: s1[i] against s2[k + i], offset -k
    for (uint32_t k = 0; k + kClOverlapReq < len2; ++k) {
        const uint32_t ol = min(len1, len2 - k), n = min(kClOverlapCmp, ol), lim = min(5u, ol / 5);
        if (cl_mism(w1_0, w2, n) <= lim) {
            *off_out = -static_cast<int>(k);
            *ol_out = ol;
            return true;
        }
        const uint32_t j = k + kClOverlapCmp;
        if (j < len2) cl_push(w2, cl_comp(p2[len2 - 1 - j])); else cl_push_none(w2);
    }
    return false;
}

// fastp's trimPolyG (min length 10), on p[0 .. len): the new length
__device__ inline uint32_t cl_poly_g(const uint8_t* p, uint32_t len) {
    uint32_t mism = 0, first_g = len - 1, i = 0;   // (len 0: the loop does not run, i = 0 < 10)
    for (; i < len; ++i) {
        if (p[len - 1 - i] != 'G') ++mism; else first_g = len - 1 - i;
        if (mism > 5 || (mism > (i + 1) / 8 && i >= 9)) break;
    }
    return i >= 10 ? first_g : len;
}

// ------------------------------------------------------------------ kernels --

__global__ void __launch_bounds__(kClThreads) vk_cl_init_kernel(const ClSample* samples, uint32_t nsamples,
                                                                const ClFile* files, uint32_t nfiles, ClRec* recs,
                                                                uint64_t* stats, uint32_t nstat, uint32_t* status) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t < nsamples) status[t] = samples[t].flags;
    if (t < nfiles && files[t].nrec) recs[files[t].rec0].h = files[t].off;
    for (uint64_t i = t; i < static_cast<uint64_t>(nsamples) * nstat; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        stats[i] = 0;
}

// newlines of this lane's 64 bytes at `pos` of a file of `len` bytes (bytes at and past `len` not counted); the bytes
// are kept in w
__device__ inline uint32_t cl_lane_newlines(const uint8_t* file, uint64_t len, uint64_t pos, uint32_t w[16]) {
    uint32_t cnt = 0;
    for (uint32_t q = 0; q < 4; ++q) {
        const uint64_t p = pos + q * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (p < len) v = *reinterpret_cast<const uint4*>(file + p);   // (16-byte aligned; readable to the rounded end)
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t pj = p + 4 * j;
            uint32_t m = cl_nl_in(w[4 * q + j]);
            if (pj >= len) m = 0;
            else if (len - pj < 4) m &= (1u << (8 * (len - pj))) - 1u;
            cnt += __popc(m);
        }
    }
    return cnt;
}

// the same for chunk c of the launch: its file and the lane's position in it go to f_out / pos_out
__device__ inline uint32_t cl_chunk_lane(const uint8_t* text, const ClFile* files, const uint64_t* chunk_base,
                                         uint32_t nfiles, uint64_t c, uint32_t* f_out, uint64_t* pos_out, uint32_t w[16]) {
    const uint32_t f = cl_find_u64(chunk_base, nfiles, c);
    const ClFile fd = files[f];
    const uint64_t pos = (c - fd.chunk0) * kClChunk + threadIdx.x * 64ull;
    *f_out = f;
    *pos_out = pos;
    return cl_lane_newlines(text + fd.off, fd.len, pos, w);
}

__global__ void __launch_bounds__(kClThreads) vk_cl_nl_count_kernel(const uint8_t* text, const ClFile* files,
                                                                    const uint64_t* chunk_base, uint32_t nfiles,
                                                                    uint64_t* counts) {
    __shared__ uint32_t part[kClThreads];
    const uint64_t c = blockIdx.x;
    uint32_t f, w[16];
    uint64_t pos;
    part[threadIdx.x] = cl_chunk_lane(text, files, chunk_base, nfiles, c, &f, &pos, w);
    __syncthreads();
    for (uint32_t s = kClThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[c] = part[0];
}

// per-file line counts for vk_clean_lines_device (one atomic per chunk)
__global__ void __launch_bounds__(kClThreads) vk_cl_lines_kernel(const uint8_t* text, const ClFile* files,
                                                                const uint64_t* chunk_base, uint32_t nfiles,
                                                                unsigned long long* lines) {
    __shared__ uint32_t part[kClThreads];
    const uint64_t c = blockIdx.x;
    uint32_t f, w[16];
    uint64_t pos;
    part[threadIdx.x] = cl_chunk_lane(text, files, chunk_base, nfiles, c, &f, &pos, w);
    __syncthreads();
    for (uint32_t s = kClThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(lines + f, static_cast<unsigned long long>(part[0]));
}

// The read-length head of a file for vk_clean_heads_device: what avg_read_length (rawinput.py) sums over the whole text.
// Its fragments are what lies between newlines; fragment i has i newlines ahead of it, the last one ends with the
// file (and is empty when the file ends in a newline).  Fragments 4j + 1 with j < sample_size count, each with its
// length less the whitespace at both ends.  That length is (end - start) of two positions which different lanes
// find: the lane that holds newline 4j walks forward from the byte after it to the first byte that is no
// whitespace (or the fragment's end) and subtracts that position; the lane that holds newline 4j + 1 walks back
// from it over whitespace and adds where it stops -- or, when the walk reaches the fragment's start, the
// fragment's end: the forward walk of an all-whitespace fragment stopped there too.  Sums are modulo 2^64.
__device__ inline bool cl_space(uint8_t b) { return b == ' ' || (b >= '\t' && b <= '\r'); }   // bytes.strip()'s set

__device__ inline uint64_t cl_head_start(const uint8_t* file, uint64_t len, uint64_t q) {
    while (q < len && file[q] != '\n' && cl_space(file[q])) ++q;
    return q;
}

__device__ inline uint64_t cl_head_end(const uint8_t* file, uint64_t e) {
    uint64_t q = e;
    while (q > 0 && file[q - 1] != '\n' && cl_space(file[q - 1])) --q;
    return (q == 0 || file[q - 1] == '\n') ? e : q;
}

// One workgroup per file, from the file's start in kClChunk pieces until the newline that ends fragment
// 4 (sample_size - 1) + 1 has been seen or the file ends: a file costs its first sample_size records, whatever its size.
__global__ void __launch_bounds__(kClThreads) vk_cl_heads_kernel(const uint8_t* text, const uint64_t* offsets,
                                                                const uint64_t* lengths, uint32_t sample_size,
                                                                uint64_t* totals, uint64_t* counted) {
    __shared__ uint32_t wave_sum[kClThreads / 64];
    __shared__ uint64_t part[kClThreads];
    const uint32_t f = blockIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const uint8_t* file = text + offsets[f];
    const uint64_t len = lengths[f];
    const uint64_t want = 4ull * sample_size - 2;   // newlines up to the end of the last fragment that counts
    uint64_t seen = 0, acc = 0;                     // newlines ahead of this chunk (the same in every lane); this lane's sum
    for (uint64_t c0 = 0; c0 < len && seen < want; c0 += kClChunk) {
        const uint64_t pos = c0 + threadIdx.x * 64ull;
        uint32_t w[16];
        const uint32_t cnt = cl_lane_newlines(file, len, pos, w);
        uint32_t incl = cnt;   // newlines of this wavefront's lanes up to this one, then of the waves ahead
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t ahead = 0, total = 0;
        for (uint32_t v = 0; v < kClThreads / 64; ++v) {
            if (v < wave) ahead += wave_sum[v];
            total += wave_sum[v];
        }
        __syncthreads();   // (wave_sum is written again in the next round)
        uint64_t line = seen + ahead + incl - cnt;   // index of the fragment that this lane's first newline ends
        if (cnt && line < want) {
            for (uint32_t b = 0; b < 64; ++b) {
                if (((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) != '\n') continue;
                const uint64_t p = pos + b;
                if (p >= len || line >= want) break;
                if ((line & 3) == 0) acc -= cl_head_start(file, len, p + 1);
                else if ((line & 3) == 1) acc += cl_head_end(file, p);
                ++line;
            }
        }
        seen += total;
    }
    // the fragment that the end of the file ends
    if (threadIdx.x == 0 && seen < want && (seen & 3) == 1) acc += cl_head_end(file, len);
    part[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t s = kClThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint64_t n = (seen + 3) / 4;   // fragments 4j + 1 among 0 .. seen
        totals[f] = part[0];
        counted[f] = n < sample_size ? n : sample_size;
    }
}

// exclusive scan of u64 items, three phases: block sums, one block over the sums, blocks again
__device__ inline uint64_t cl_block_exclusive(uint64_t v, uint64_t* sh, uint64_t* total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kClThreads; d <<= 1) {
        const uint64_t add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const uint64_t incl = sh[threadIdx.x];
    *total = sh[kClThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(kClThreads) vk_cl_scan_reduce_kernel(const uint64_t* in, uint64_t n, uint64_t* sums) {
    __shared__ uint64_t sh[kClThreads];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kClScanBlock + threadIdx.x * kClScanItems;
    uint64_t s = 0;
    for (uint32_t i = 0; i < kClScanItems; ++i)
        if (base + i < n) s += in[base + i];
    uint64_t total;
    cl_block_exclusive(s, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kClThreads) vk_cl_scan_top_kernel(uint64_t* sums, uint64_t nb) {
    __shared__ uint64_t sh[kClThreads];
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < nb; t0 += kClThreads) {
        const uint64_t i = t0 + threadIdx.x;
        const uint64_t v = i < nb ? sums[i] : 0;
        uint64_t total;
        const uint64_t ex = cl_block_exclusive(v, sh, &total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) sums[nb] = carry;
}

__global__ void __launch_bounds__(kClThreads) vk_cl_scan_apply_kernel(const uint64_t* in, uint64_t n, const uint64_t* sums,
                                                                     uint64_t* out) {
    __shared__ uint64_t sh[kClThreads];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kClScanBlock + threadIdx.x * kClScanItems;
    uint64_t s = 0;
    for (uint32_t i = 0; i < kClScanItems; ++i)
        if (base + i < n) s += in[base + i];
    uint64_t total;
    uint64_t run = sums[blockIdx.x] + cl_block_exclusive(s, sh, &total);
    for (uint32_t i = 0; i < kClScanItems; ++i)
        if (base + i < n) {
            const uint64_t v = in[base + i];
            out[base + i] = run;
            run += v;
        }
    if (base < n && base + kClScanItems >= n) out[n] = run;   // (the lane that holds the last item)
}

__global__ void __launch_bounds__(kClThreads) vk_cl_nl_write_kernel(const uint8_t* text, const ClFile* files,
                                                                    const uint64_t* chunk_base, uint32_t nfiles,
                                                                    const uint64_t* nl_prefix, ClRec* recs) {
    __shared__ uint64_t sh[kClThreads];
    const uint64_t c = blockIdx.x;
    uint32_t f, w[16];
    uint64_t pos;
    const uint32_t cnt = cl_chunk_lane(text, files, chunk_base, nfiles, c, &f, &pos, w);
    uint64_t total;
    const uint64_t ex = cl_block_exclusive(cnt, sh, &total);
    if (cnt == 0) return;
    const ClFile fd = files[f];
    uint64_t line = nl_prefix[c] - nl_prefix[fd.chunk0] + ex;   // line index (in the file) of this lane's first newline
    const uint64_t lines = 4 * fd.nrec;
    if (line >= lines) return;
    for (uint32_t b = 0; b < 64; ++b) {
        const uint64_t p = pos + b;
        if (p >= fd.len) break;
        if (((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) != '\n') continue;
        if (line < lines) {
            const uint64_t r = line >> 2, at = fd.off + p;
            ClRec* rec = recs + fd.rec0 + r;
            switch (line & 3) {
                case 0: rec->he = at; break;
                case 1: rec->se = at; break;
                case 2: rec->pe = at; break;
                default:
                    rec->qe = at;
                    if (r + 1 < fd.nrec) rec[1].h = at + 1;
                    break;
            }
        }
        ++line;
    }
}

__device__ inline bool cl_rec_ok(const uint8_t* text, const ClRec& r) {
    const uint64_t bad = ~0ull;
    if (r.h == bad || r.he == bad || r.se == bad || r.pe == bad || r.qe == bad) return false;
    if (!(r.h < r.he && r.he < r.se && r.se < r.pe && r.pe < r.qe)) return false;
    if (text[r.h] != '@' || text[r.se + 1] != '+') return false;
    return r.qe - r.pe == r.se - r.he;
}

__device__ inline uint64_t cl_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ inline uint64_t cl_hash_bytes(uint64_t h, const uint8_t* p, uint64_t n) {
    h = cl_mix(h ^ n);
    for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

__device__ inline uint32_t cl_unit_sample(const uint64_t* unit_base, uint32_t nsamples, uint64_t u) {
    return cl_find_u64(unit_base, nsamples, u);
}

// records of unit u: (r1, r2 or ~0)
__device__ inline void cl_unit_recs(const ClSample& s, uint64_t k, uint64_t* r1, uint64_t* r2) {
    if (k < s.npairs) {
        *r1 = s.r1 + k;
        *r2 = s.r2 + k;
    } else {
        *r1 = s.se + (k - s.npairs);
        *r2 = ~0ull;
    }
}

__global__ void __launch_bounds__(kClThreads) vk_cl_hash_kernel(const uint8_t* text, const ClSample* samples,
                                                               const uint64_t* unit_base, uint32_t nsamples,
                                                               uint64_t nunits, const ClRec* recs, uint64_t hash_mask,
                                                               uint64_t* hashes, uint32_t* status) {
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u >= nunits) return;
    const uint32_t si = cl_unit_sample(unit_base, nsamples, u);
    const ClSample s = samples[si];
    uint64_t r1, r2;
    cl_unit_recs(s, u - unit_base[si], &r1, &r2);
    const ClRec a = recs[r1];
    bool ok = cl_rec_ok(text, a);
    uint64_t h = cl_mix(0x5EEDull + 2ull * si + (r2 != ~0ull ? 1u : 0u));
    if (ok) h = cl_hash_bytes(h, text + a.he + 1, a.se - a.he - 1);
    if (r2 != ~0ull) {
        const ClRec b = recs[r2];
        const bool ok2 = cl_rec_ok(text, b);
        if (ok && ok2) h = cl_hash_bytes(h, text + b.he + 1, b.se - b.he - 1);
        ok = ok && ok2;
    }
    if (!ok) atomicOr(status + si, 1u);   // VK_CL_BAD_FRAMING
    hashes[u] = cl_mix(h) & hash_mask;
}

__device__ inline bool cl_same_bytes(const uint8_t* text, const ClRec& a, const ClRec& b) {
    const uint64_t n = a.se - a.he - 1;
    if (b.se - b.he - 1 != n) return false;
    const uint8_t* p = text + a.he + 1;
    const uint8_t* q = text + b.he + 1;
    for (uint64_t i = 0; i < n; ++i)
        if (p[i] != q[i]) return false;
    return true;
}

__global__ void __launch_bounds__(kClThreads) vk_cl_dedup_kernel(const uint8_t* text, const ClSample* samples,
                                                                const uint64_t* unit_base, uint32_t nsamples,
                                                                uint64_t nunits, const ClRec* recs,
                                                                const uint64_t* hashes, const uint32_t* status,
                                                                uint32_t* table, uint64_t slot_mask, uint32_t* slot_of) {
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u >= nunits) return;
    const uint32_t si = cl_unit_sample(unit_base, nsamples, u);
    if (status[si]) return;
    const ClSample s = samples[si];
    const uint64_t k = u - unit_base[si];
    uint64_t r1, r2;
    cl_unit_recs(s, k, &r1, &r2);
    const bool paired = r2 != ~0ull;
    const uint64_t h = hashes[u];
    uint64_t slot = h & slot_mask;
    // table[2 slot] = representative unit (kClEmpty: free), table[2 slot + 1] = least unit of the class
    for (;;) {
        uint32_t rep = __hip_atomic_load(table + 2 * slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (rep == kClEmpty) {
            rep = atomicCAS(table + 2 * slot, kClEmpty, static_cast<uint32_t>(u));
            if (rep == kClEmpty) break;   // a new class, represented by u
        }
        if (hashes[rep] == h) {
            // same group: the same sample (unit range) and the same kind (pair / single)
            const uint64_t rk = static_cast<uint64_t>(rep) - unit_base[si];
            const bool same_group = rep >= unit_base[si] && rep < unit_base[si + 1] && ((rk < s.npairs) == paired);
            if (same_group) {
                uint64_t q1, q2;
                cl_unit_recs(s, rk, &q1, &q2);
                if (cl_same_bytes(text, recs[r1], recs[q1]) && (!paired || cl_same_bytes(text, recs[r2], recs[q2]))) break;
            }
        }
        slot = (slot + 1) & slot_mask;
    }
    atomicMin(table + 2 * slot + 1, static_cast<uint32_t>(u));
    slot_of[u] = static_cast<uint32_t>(slot);
}

// trim F / T; false: the read is discarded (F + T > length)
__device__ inline bool cl_trim(uint32_t len, uint32_t F, uint32_t T, uint32_t* a, uint32_t* l) {
    if (F + T > len) return false;
    *a = F;
    *l = len - F - T;
    return true;
}

// an adapter of vk_clean_adapters_device: 2-bit codes (A0 C1 T2 G3, as ClWin) at the even bits of lo (positions 0..31)
// and hi (32..63), non-ACGT flags at the same bits; len 0: none
constexpr uint32_t kClMaxAdapter = 64;
struct ClAdapter {
    uint64_t lo, hi, nlo, nhi;
    uint32_t len, pad;
    uint8_t seq[kClMaxAdapter];
};

// trimming by sequence (vk_adapter.h, after this file in the translation unit)
__device__ inline uint32_t cl_seq_cut(const uint8_t* p, uint32_t len, const ClAdapter* ad, uint32_t* nread, uint32_t* nbase);

// kSeq: vk_clean_adapters_device -- adapters[3 sample + group] (R1, R2, single reads) trim by sequence, and the reads /
// bases they cut go to ad_stats[2 sample + 0 / 1]; without it (vk_clean_device) both are unused
template <bool kSeq>
__global__ void __launch_bounds__(kClThreads) vk_cl_clean_kernel(const uint8_t* text, const ClSample* samples,
                                                                const uint64_t* unit_base, uint32_t nsamples,
                                                                uint64_t nunits, const ClRec* recs,
                                                                const uint32_t* status, const uint32_t* table,
                                                                const uint32_t* slot_of, uint32_t F, uint32_t T,
                                                                uint32_t flags, ClPlan* plans, uint64_t* out_bytes,
                                                                const ClAdapter* adapters, uint64_t* ad_stats) {
    const uint64_t u = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if constexpr (!kSeq) {
        if (u >= nunits) return;
    }
    uint32_t si = 0, nread = 0, nbase = 0;   // (kSeq: reads and bases of this unit cut by sequence)
    if (u < nunits) {
        si = cl_unit_sample(unit_base, nsamples, u);
        ClPlan pl = {};
        uint64_t bytes = 0;
        bool keep = status[si] == 0;
        if (keep && (flags & 4u)) keep = table[2ull * slot_of[u] + 1] == static_cast<uint32_t>(u);   // VK_CL_DEDUP
        if (keep) {
            const ClSample s = samples[si];
            uint64_t r1, r2;
            cl_unit_recs(s, u - unit_base[si], &r1, &r2);
            const ClRec a = recs[r1];
            const uint8_t* s1 = text + a.he + 1;
            const uint32_t len1 = static_cast<uint32_t>(a.se - a.he - 1);
            if (r2 == ~0ull) {
                if (cl_trim(len1, F, T, &pl.a1, &pl.l1)) {
                    pl.l1 = cl_poly_g(s1 + pl.a1, pl.l1);
                    if constexpr (kSeq) {
                        if (flags & 1u) pl.l1 = cl_seq_cut(s1 + pl.a1, pl.l1, adapters + 3ull * si + 2, &nread, &nbase);
                    }
                    if (pl.l1) {
                        pl.flags = 1;
                        bytes = (a.he - a.h) + 2ull * pl.l1 + 5;
                    }
                }
            } else {
                const ClRec b = recs[r2];
                const uint8_t* s2 = text + b.he + 1;
                const uint32_t len2 = static_cast<uint32_t>(b.se - b.he - 1);
                if (cl_trim(len1, F, T, &pl.a1, &pl.l1) && cl_trim(len2, F, T, &pl.a2, &pl.l2)) {
                    pl.l1 = cl_poly_g(s1 + pl.a1, pl.l1);
                    pl.l2 = cl_poly_g(s2 + pl.a2, pl.l2);
                    int off;
                    uint32_t ol;
                    bool cut = false;
                    if ((flags & 1u) && cl_overlap(s1 + pl.a1, pl.l1, s2 + pl.a2, pl.l2, &off, &ol) && off < 0) {   // VK_CL_ADAPTER
                        pl.l1 = min(pl.l1, ol + F);
                        pl.l2 = min(pl.l2, ol + F);
                        cut = true;
                    }
                    if constexpr (kSeq) {
                        if ((flags & 1u) && !cut) {   // the overlap did not cut the pair: each mate by its adapter
                            pl.l1 = cl_seq_cut(s1 + pl.a1, pl.l1, adapters + 3ull * si, &nread, &nbase);
                            pl.l2 = cl_seq_cut(s2 + pl.a2, pl.l2, adapters + 3ull * si + 1, &nread, &nbase);
                        }
                    }
                    if ((flags & 2u) && cl_overlap(s1 + pl.a1, pl.l1, s2 + pl.a2, pl.l2, &off, &ol)) {    // VK_CL_MERGE
                        pl.m1 = ol + (off > 0 ? static_cast<uint32_t>(off) : 0u);
                        pl.t0 = ol;
                        pl.m2 = off > 0 ? pl.l2 - ol : 0u;
                        if (pl.m1 + pl.m2) {
                            pl.flags = 1 | 4;
                            bytes = (a.he - a.h) + 2ull * (pl.m1 + pl.m2) + 5;
                        }
                    } else {
                        if (pl.l1) {
                            pl.flags |= 1;
                            bytes += (a.he - a.h) + 2ull * pl.l1 + 5;
                        }
                        if (pl.l2) {
                            pl.flags |= 2;
                            bytes += (b.he - b.h) + 2ull * pl.l2 + 5;
                        }
                    }
                }
            }
        }
        plans[u] = pl;
        out_bytes[u] = bytes;
    }
    if constexpr (kSeq) {
        // the workgroup's first sample: summed in LDS, one global add; a unit of another sample adds its own
        __shared__ uint64_t red[2][kClThreads];
        const uint32_t s0 = cl_unit_sample(unit_base, nsamples, static_cast<uint64_t>(blockIdx.x) * blockDim.x);
        const bool local = u < nunits && si == s0;
        if (!local && nread) {
            atomicAdd(reinterpret_cast<unsigned long long*>(ad_stats + 2ull * si), static_cast<unsigned long long>(nread));
            atomicAdd(reinterpret_cast<unsigned long long*>(ad_stats + 2ull * si + 1), static_cast<unsigned long long>(nbase));
        }
        red[0][threadIdx.x] = local ? nread : 0;
        red[1][threadIdx.x] = local ? nbase : 0;
        __syncthreads();
        for (uint32_t s = kClThreads / 2; s > 0; s >>= 1) {
            if (threadIdx.x < s) {
                red[0][threadIdx.x] += red[0][threadIdx.x + s];
                red[1][threadIdx.x] += red[1][threadIdx.x + s];
            }
            __syncthreads();
        }
        if (threadIdx.x < 2 && red[threadIdx.x][0])
            atomicAdd(reinterpret_cast<unsigned long long*>(ad_stats + 2ull * s0 + threadIdx.x),
                      static_cast<unsigned long long>(red[threadIdx.x][0]));
    }
}

// the wave's copy of n bytes: out[i] = f(i), lanes take consecutive bytes
template <typename F>
__device__ inline void cl_wave_copy(uint8_t* out, uint32_t n, uint32_t lane, F f) {
    for (uint32_t i = lane; i < n; i += 64) out[i] = f(i);
}

struct ClCycles {   // LDS: per-cycle base counts of the workgroup's first sample, and its bases / records per wavefront
    uint32_t base[kClCycles][4];
    uint32_t reach[kClCycles];
    uint64_t bp[kClThreads / 64], recs[kClThreads / 64];
};

__device__ inline void cl_count_cycles(ClCycles* lds, uint64_t* gstats, bool local, uint8_t b, uint32_t i) {
    // i < kClCycles; codes A C G T -> 0 1 2 3
    const int c = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1;
    if (local) {
        atomicAdd(&lds->reach[i], 1u);
        if (c >= 0) atomicAdd(&lds->base[i][c], 1u);
    } else {
        atomicAdd(reinterpret_cast<unsigned long long*>(gstats + 2 + 4 * kClCycles + i), 1ull);
        if (c >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(gstats + 2 + 4 * i + c), 1ull);
    }
}

__global__ void __launch_bounds__(kClThreads) vk_cl_write_kernel(const uint8_t* text, const ClSample* samples,
                                                                const uint64_t* unit_base, uint32_t nsamples,
                                                                uint64_t nunits, const ClRec* recs, const ClPlan* plans,
                                                                const uint64_t* out_prefix, uint8_t* out,
                                                                uint64_t* stats, uint32_t nstat) {
    __shared__ ClCycles lds;
    for (uint32_t i = threadIdx.x; i < kClCycles * 5; i += kClThreads) {
        if (i < 4 * kClCycles) lds.base[i / 4][i % 4] = 0; else lds.reach[i - 4 * kClCycles] = 0;
    }
    __syncthreads();
    const uint64_t u0 = static_cast<uint64_t>(blockIdx.x) * kClUnitsPerBlock;
    const uint32_t s0 = u0 < nunits ? cl_unit_sample(unit_base, nsamples, u0) : 0;
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    // (the workgroup's own sample: bases and records summed in registers, not by atomics on one LDS word -- those
    // the compiler turns into a loop of lane reads inside this divergent loop)
    uint64_t own_bp = 0, own_recs = 0;
    for (uint32_t j = wave; j < kClUnitsPerBlock; j += kClThreads / 64) {
        const uint64_t u = u0 + j;
        if (u >= nunits) break;
        const ClPlan pl = plans[u];
        if (!pl.flags) continue;
        const uint32_t si = cl_unit_sample(unit_base, nsamples, u);
        const ClSample s = samples[si];
        const uint64_t k = u - unit_base[si];
        uint64_t r1, r2;
        cl_unit_recs(s, k, &r1, &r2);
        const bool local = si == s0;
        uint64_t* gs = stats + static_cast<uint64_t>(si) * nstat;
        // the base-frequency group: the pairs (merged reads, else R1) if the sample has any, else the single reads
        const bool cyc = s.npairs ? k < s.npairs : true;
        uint8_t* o = out + s.out_off + (out_prefix[u] - out_prefix[unit_base[si]]);
        uint64_t bp = 0, nrec = 0;
        const ClRec a = recs[r1];
        const uint8_t* q1 = text + a.pe + 1;
        const uint8_t* s1 = text + a.he + 1;
        for (uint32_t m = 0; m < 2; ++m) {
            if (!(pl.flags & (1u << m))) continue;
            const ClRec rc = m == 0 ? a : recs[r2];
            const uint8_t* sq = text + rc.he + 1 + (m == 0 ? pl.a1 : pl.a2);
            const uint8_t* qq = text + rc.pe + 1 + (m == 0 ? pl.a1 : pl.a2);
            const uint32_t hl = static_cast<uint32_t>(rc.he - rc.h);
            cl_wave_copy(o, hl, lane, [&](uint32_t i) { return text[rc.h + i]; });
            o += hl;
            if (lane == 0) o[0] = '\n';
            o += 1;
            uint32_t L;
            if (m == 0 && (pl.flags & 4u)) {
                // merged: R1 kept [0, m1) then rc(R2 kept)[t0, t0 + m2); qualities R1's, then R2's reversed
                const ClRec b = recs[r2];
                const uint8_t* s2 = text + b.he + 1 + pl.a2;
                const uint8_t* q2 = text + b.pe + 1 + pl.a2;
                const uint32_t m1 = pl.m1, t0 = pl.t0, l2 = pl.l2;
                L = m1 + pl.m2;
                cl_wave_copy(o, L, lane, [&](uint32_t i) { return i < m1 ? s1[pl.a1 + i] : cl_comp(s2[l2 - 1 - (t0 + i - m1)]); });
                cl_wave_copy(o + L + 3, L, lane, [&](uint32_t i) { return i < m1 ? q1[pl.a1 + i] : q2[l2 - 1 - (t0 + i - m1)]; });
            } else {
                L = m == 0 ? pl.l1 : pl.l2;
                cl_wave_copy(o, L, lane, [&](uint32_t i) { return sq[i]; });
                cl_wave_copy(o + L + 3, L, lane, [&](uint32_t i) { return qq[i]; });
            }
            if (cyc && m == 0 && lane < kClCycles && lane < L) cl_count_cycles(&lds, gs, local, o[lane], lane);
            if (lane == 0) {
                o[L] = '\n';
                o[L + 1] = '+';
                o[L + 2] = '\n';
                o[2 * L + 3] = '\n';
            }
            o += 2ull * L + 4;
            bp += L;
            ++nrec;
        }
        if (local) {
            own_bp += bp;
            own_recs += nrec;
        } else if (lane == 0) {
            atomicAdd(reinterpret_cast<unsigned long long*>(gs), static_cast<unsigned long long>(bp));
            atomicAdd(reinterpret_cast<unsigned long long*>(gs + 1), static_cast<unsigned long long>(nrec));
        }
    }
    if (lane == 0) {
        lds.bp[wave] = own_bp;
        lds.recs[wave] = own_recs;
    }
    __syncthreads();
    if (u0 >= nunits) return;
    uint64_t* gs = stats + static_cast<uint64_t>(s0) * nstat;
    for (uint32_t i = threadIdx.x; i < 5 * kClCycles + 2; i += kClThreads) {
        uint64_t v = 0;
        uint64_t* dst;
        if (i < 4 * kClCycles) { v = lds.base[i / 4][i % 4]; dst = gs + 2 + i; }
        else if (i < 5 * kClCycles) { v = lds.reach[i - 4 * kClCycles]; dst = gs + 2 + i; }
        else {
            const bool is_bp = i == 5 * kClCycles;
            for (uint32_t w = 0; w < kClThreads / 64; ++w) v += is_bp ? lds.bp[w] : lds.recs[w];
            dst = is_bp ? gs : gs + 1;
        }
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(dst), static_cast<unsigned long long>(v));
    }
}

__global__ void __launch_bounds__(kClThreads) vk_cl_finish_kernel(const ClSample* samples, const uint64_t* unit_base,
                                                                 uint32_t nsamples, const uint64_t* out_prefix,
                                                                 const uint32_t* status, uint8_t* out,
                                                                 uint64_t* out_lengths) {
    const uint32_t si = blockIdx.x;
    if (si >= nsamples) return;
    const ClSample s = samples[si];
    const uint64_t n = status[si] ? 0 : out_prefix[unit_base[si + 1]] - out_prefix[unit_base[si]];
    if (threadIdx.x == 0) out_lengths[si] = n;
    const uint64_t end = (n + 15) / 16 * 16;
    for (uint64_t i = n + threadIdx.x; i < end; i += blockDim.x) out[s.out_off + i] = 0;
}

#endif  // VK_TEXT_STRUCTS_ONLY

}  // namespace

#endif  // VK_CLEAN_H
