// vk_emit.h -- step C's files: the reads that each step of the subsample ladder takes, written as FASTQ text in HBM
// (split_fastq / run_parallel_reformats, commands/image.py:577-725: one `reformat.sh samplebasestarget=...` per size).
// Part of the one translation unit vkimg.hip (device code for gfx950; see the notes there).
//
// The rule is tests/ladder_emit_ref.py ("Step C"): a step takes the reads the walker of vk_ladder.h
// counts for it (sample_hash(seed, anchor) < threshold, the anchor the sample offset of the newline that ends the
// header line), in input order; a record is four lines, each ended by one '\n' (a trailing '\r' dropped, the third
// line a bare '+'); every sequence byte outside ACGTacgt becomes 'N'; a read of more than 500 bases of a sampled step
// is cut into pieces of 500 (reformat.sh's breaklength=500), each a record named `<header>_<n>`; a whole step writes
// every record uncut.  Counting a step's text gives the histogram that the direct run counted for the step.
//
// Launch sequence of vk_ladder_emit_device (a lane or a wave per item, no grid-wide barrier inside a kernel):
//   vk_cl_nl_count / vk_cl_scan_* / vk_cl_nl_write   step B's record index (vk_clean.h): a sample is one file,
//                            every line end goes to its record
//   vk_em_status_kernel      per sample: framing as the read index states it (VK_ST_*), size, the caller's record count
//   vk_em_plan_kernel        per item = (step, record of its sample): one hash; the bytes the record gives the step
//   vk_cl_scan_*             exclusive scan of the items' bytes: an item's place in its step's file
//   vk_em_sizes_kernel       per step: its file's length (the host lays the files out at multiples of 16 bytes and
//                            stops here when they do not fit)
//   vk_em_write_kernel       wave per item: the record or its pieces, lanes on consecutive bytes
//   vk_em_pad_kernel         per step: zeros up to the file's 16-byte rounded end
#ifndef VK_EMIT_H
#define VK_EMIT_H

#include "vk_clean.h"
#include "vk_lane.h"

namespace {

constexpr uint32_t kEmItemsPerBlock = 64;             // items per workgroup of the write kernel (16 per wavefront)
constexpr uint32_t kEmStartScan = 65536;              // vk_check_kernel looks for the first '+' line this far
constexpr uint32_t kEmBadSize = 4u, kEmBadRecords = 8u;   // VK_EM_TOO_LARGE, VK_EM_BAD_RECORDS (vkimg.h)

struct EmSample {
    uint64_t off, len;       // text in d_fastq
    uint64_t rec0, nrec;     // its records in the index
    uint64_t chunk0, chunk1; // its chunks of the newline passes
};

struct EmStep {
    uint64_t seed, threshold;
    uint64_t out_off;        // where its file starts in d_out (known after the scan)
    uint32_t sample, whole;
};

#ifndef VK_TEXT_STRUCTS_ONLY   // (vk_clean.h: the plain structs above are all a host compiler takes)

struct EmRec {               // a record's lines without their '\r': header [h, h + hl), sequence [s, s + L), quality [q, q + Lq)
    uint64_t h, s, q;
    uint32_t hl, L, Lq;
};

__device__ inline EmRec em_rec(const uint8_t* text, const ClRec& r, uint64_t end) {
    const uint64_t qe = r.qe == ~0ull ? end : r.qe;   // (the sample's last line may lack its newline)
    EmRec g;
    g.h = r.h;
    g.s = r.he + 1;
    g.q = r.pe + 1;
    g.hl = static_cast<uint32_t>(r.he - r.h);
    g.L = static_cast<uint32_t>(r.se - g.s);
    g.Lq = static_cast<uint32_t>(qe - g.q);
    if (g.hl && text[r.he - 1] == '\r') --g.hl;
    if (g.L && text[r.se - 1] == '\r') --g.L;
    if (g.Lq && text[qe - 1] == '\r') --g.Lq;
    return g;
}

__device__ inline uint32_t em_digits(uint32_t n) {   // decimal width of n
    uint32_t d = 1;
    for (uint64_t p = 10; d < 10 && n >= p; p *= 10) ++d;
    return d;
}

__device__ inline uint64_t em_digits_sum(uint32_t n) {   // decimal widths of 1 .. n together
    uint64_t sum = 0, lo = 1;
    for (uint32_t d = 1; d <= 10 && lo <= n; ++d) {
        const uint64_t hi = min(static_cast<uint64_t>(n), lo * 10 - 1);
        sum += d * (hi - lo + 1);
        lo *= 10;
    }
    return sum;
}

__device__ inline uint8_t em_base(uint8_t b) {   // reformat.sh's iupacToN, for every byte that is no base; case kept
    const uint8_t l = b | 0x20;
    return (l == 'a' || l == 'c' || l == 'g' || l == 't') ? b : static_cast<uint8_t>('N');
}

// ------------------------------------------------------------------ kernels --

__global__ void __launch_bounds__(kClThreads) vk_em_status_kernel(const uint8_t* text, const EmSample* samples,
                                                                 uint32_t nsamples, const ClRec* recs,
                                                                 const uint64_t* nl_prefix, uint32_t* status) {
    const uint32_t si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= nsamples) return;
    const EmSample s = samples[si];
    uint32_t st = 0;
    if (s.len >= (1ull << 32)) st |= kEmBadSize;   // (anchors are 32-bit offsets, as in the read index)
    if (s.len) {
        const uint8_t* p = text + s.off;
        if (p[0] != '@') st |= VK_ST_BAD_START;
        const uint64_t lines = nl_prefix[s.chunk1] - nl_prefix[s.chunk0] + (p[s.len - 1] != '\n' ? 1u : 0u);
        if (lines & 3u) st |= VK_ST_BAD_PHASE;
        else if (lines != 4 * s.nrec) st |= kEmBadRecords;
        if (s.nrec) {
            const uint64_t se = recs[s.rec0].se;   // the sample's second newline
            if (se != ~0ull && se - s.off < kEmStartScan && se + 1 < s.off + s.len && text[se + 1] != '+') st |= VK_ST_BAD_START;
        }
    }
    status[si] = st;
}

__global__ void __launch_bounds__(kClThreads) vk_em_plan_kernel(const uint8_t* text, const EmSample* samples,
                                                               const EmStep* steps, const uint64_t* step_base,
                                                               uint32_t nsteps, uint64_t nitems, const ClRec* recs,
                                                               const uint32_t* status, uint64_t* out_bytes) {
    const uint64_t item = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (item >= nitems) return;
    const uint32_t st = cl_find_u64(step_base, nsteps, item);
    const EmStep step = steps[st];
    uint64_t bytes = 0;
    if (status[step.sample] == 0) {
        const EmSample s = samples[step.sample];
        const ClRec r = recs[s.rec0 + (item - step_base[st])];
        if (step.whole || vkl::sample_take(step.seed, r.he - s.off, step.threshold)) {
            const EmRec g = em_rec(text, r, s.off + s.len);
            if (step.whole || g.L <= vkl::kBreakLength) {
                bytes = 5ull + g.hl + g.L + g.Lq;
            } else {
                const uint32_t pieces = (g.L + vkl::kBreakLength - 1) / vkl::kBreakLength;
                bytes = static_cast<uint64_t>(pieces) * (g.hl + 6ull) + em_digits_sum(pieces) + g.L + min(g.Lq, g.L);
            }
        }
    }
    out_bytes[item] = bytes;
}

__global__ void __launch_bounds__(kClThreads) vk_em_sizes_kernel(const uint64_t* step_base, uint32_t nsteps,
                                                                const uint64_t* prefix, uint64_t* sizes) {
    const uint32_t st = blockIdx.x * blockDim.x + threadIdx.x;
    if (st < nsteps) sizes[st] = prefix[step_base[st + 1]] - prefix[step_base[st]];
}

// One record at o: the header (piece n > 0: with `_<n>`), sl sequence bytes from s0, '+', ql quality bytes from q0.
__device__ inline uint8_t* em_put(uint8_t* o, const uint8_t* text, const EmRec& g, uint32_t n, uint32_t s0, uint32_t sl,
                                  uint32_t q0, uint32_t ql, uint32_t lane) {
    const uint8_t* hp = text + g.h;
    cl_wave_copy(o, g.hl, lane, [&](uint32_t i) { return hp[i]; });
    o += g.hl;
    if (n) {
        const uint32_t d = em_digits(n);
        if (lane == 0) o[0] = '_';
        if (lane < d) {
            uint32_t v = n;
            for (uint32_t t = lane + 1; t < d; ++t) v /= 10;   // (d <= 10)
            o[1 + lane] = static_cast<uint8_t>('0' + v % 10);
        }
        o += 1 + d;
    }
    const uint8_t* sp = text + g.s + s0;
    const uint8_t* qp = text + g.q + q0;
    cl_wave_copy(o + 1, sl, lane, [&](uint32_t i) { return em_base(sp[i]); });
    cl_wave_copy(o + sl + 4, ql, lane, [&](uint32_t i) { return qp[i]; });
    if (lane == 0) {
        o[0] = '\n';
        o[sl + 1] = '\n';
        o[sl + 2] = '+';
        o[sl + 3] = '\n';
        o[sl + 4 + ql] = '\n';
    }
    return o + sl + ql + 5ull;
}

__global__ void __launch_bounds__(kClThreads) vk_em_write_kernel(const uint8_t* text, const EmSample* samples,
                                                                const EmStep* steps, const uint64_t* step_base,
                                                                uint32_t nsteps, uint64_t nitems, const ClRec* recs,
                                                                const uint64_t* prefix, uint8_t* out) {
    const uint64_t item0 = static_cast<uint64_t>(blockIdx.x) * kEmItemsPerBlock;
    const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (uint32_t j = wave; j < kEmItemsPerBlock; j += kClThreads / 64) {
        const uint64_t item = item0 + j;
        if (item >= nitems) break;
        const uint64_t at = prefix[item];
        if (prefix[item + 1] == at) continue;   // (the step does not take this record)
        const uint32_t st = cl_find_u64(step_base, nsteps, item);
        const EmStep step = steps[st];
        const EmSample s = samples[step.sample];
        const EmRec g = em_rec(text, recs[s.rec0 + (item - step_base[st])], s.off + s.len);
        uint8_t* o = out + step.out_off + (at - prefix[step_base[st]]);
        if (step.whole || g.L <= vkl::kBreakLength) {
            em_put(o, text, g, 0, 0, g.L, 0, g.Lq, lane);
        } else {
            const uint32_t pieces = (g.L + vkl::kBreakLength - 1) / vkl::kBreakLength;
            for (uint32_t n = 0; n < pieces; ++n) {
                const uint32_t a = n * vkl::kBreakLength, b = min(a + vkl::kBreakLength, g.L);   // [a, b) of both lines
                const uint32_t qa = min(a, g.Lq), qb = min(b, g.Lq);
                o = em_put(o, text, g, n + 1, a, b - a, qa, qb - qa, lane);
            }
        }
    }
}

__global__ void __launch_bounds__(kClThreads) vk_em_pad_kernel(const EmStep* steps, uint32_t nsteps, const uint64_t* sizes,
                                                              uint8_t* out) {
    const uint32_t st = blockIdx.x * blockDim.x + threadIdx.x;
    if (st >= nsteps) return;
    const uint64_t n = sizes[st], end = (n + 15) / 16 * 16;
    for (uint64_t i = n; i < end; ++i) out[steps[st].out_off + i] = 0;
}

#endif  // VK_TEXT_STRUCTS_ONLY

}  // namespace

#endif  // VK_EMIT_H
