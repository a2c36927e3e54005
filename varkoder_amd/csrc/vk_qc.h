// vk_qc.h -- `image / query --qc-report`: the quality profile of FASTQ streams in HBM, raw or cleaned (what fastp's
// report states before and after filtering; the reference copies those reports next to the cleaned reads,
// commands/image.py:545-547).  Part of the one translation unit vkimg.hip (device code for gfx950; see the notes there).
//
// The rule ("--qc-report: the rule"; tests/qc_ref.py is the same rule in Python, twice): a stream's first
// `records` records, four lines each as the record index frames them; a record whose sequence and quality lines differ
// in length is counted as ragged and nothing else; every other record gives its length, its bases by class (A C G T of
// either case 0..3, every other byte 4), its qualities (phred = byte - 33 clamped to 0..93) and, for the first 1,024
// cycles, base and quality sums per cycle and class.  A row is VK_QC_NSTAT u64 in the order of include/vkimg.h.
//
// Launch sequence of vk_qc_device (after the record index, vk_cl_nl_* / vk_cl_scan_*, as the emit path uses them):
//   vk_qc_status_kernel   per stream: VK_EM_BAD_RECORDS when the text holds fewer lines than 4 * records; min_length's start
//   vk_qc_count_kernel    a workgroup per kQcMerge records of ONE stream, a wavefront per record, lanes on consecutive
//                         cycles: a sequence byte and its quality byte per lane, counted into the workgroup's private
//                         tile in LDS; the tile merged into the stream's row once, at the workgroup's end
//   vk_qc_finish_kernel   per stream: VK_QC_BAD_FRAMING where a workgroup met a bad record, a row with a status zeroed,
//                         min_length of a row without counted records 0
//
// The private counters are 32 bits wide (QcTile): the per-cycle cells hold a count (10 bits) and a quality sum (22 bits)
// in one word, so a base costs two LDS additions.  They cannot overflow between merges: a workgroup counts at most
// kQcMerge <= 1023 records, a cell gains at most 1 and 93 per record, and a stream is shorter than 2^32 bytes, which bounds
// the quality histogram's cells.
//
// The lane-local code (qc_class, qc_phred, qc_lane_chunk, qc_merge) compiles for the host: tests/emul/qc_emul.cpp runs
// it, a lane at a time, against tests/qc_ref.py.  QC_ADD32 / QC_ADD64 are the additions it makes to the tile and to the
// row (atomic on the device).
#ifndef VK_QC_H
#define VK_QC_H

#include <cstdint>

#ifndef VK_QC_LANE_ONLY
#include "vk_emit.h"
#endif

// records of a workgroup = records between two merges of its private tile (the emulation shrinks it)
#ifndef VK_QC_MERGE
#define VK_QC_MERGE 512
#endif

// the additions of the lane-local code: to the tile (LDS) and to the row
#ifndef QC_ADD32
#define QC_ADD32(p, v) atomicAdd((p), (v))
#define QC_ADD64(p, v) atomicAdd(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v))
#endif

namespace {

constexpr uint32_t kQcMerge = VK_QC_MERGE;
constexpr uint32_t kQcThreads = 512;                 // 8 wavefronts share a tile
constexpr uint32_t kQcCycles = 1024, kQcPhreds = 94, kQcLenBins = 1025, kQcClasses = 5;
constexpr uint32_t kQcCopies = 32;                   // of the quality histogram: a lane adds to copy lane % 32, its own LDS bank
constexpr uint32_t kQcSumBits = 22;                  // of a cycle cell: quality sum below, count above
constexpr uint32_t kQcChunk = 256;                   // cycles a wavefront takes at a time: 4 per lane, loaded before they are counted
// a row (include/vkimg.h)
constexpr uint32_t kQcRecords = 0, kQcRagged = 1, kQcBases = 2, kQcGc = 3, kQcOther = 4, kQcMinLen = 5, kQcMaxLen = 6,
                   kQcInvalid = 7, kQcScalars = 8;
constexpr uint32_t kQcQualAt = kQcScalars, kQcReadqAt = kQcQualAt + kQcPhreds, kQcLenAt = kQcReadqAt + kQcPhreds,
                   kQcBaseAt = kQcLenAt + kQcLenBins, kQcQsumAt = kQcBaseAt + kQcCycles * kQcClasses,
                   kQcNstat = kQcQsumAt + kQcCycles * kQcClasses;
constexpr uint32_t kQcBadFraming = 16u;              // VK_QC_BAD_FRAMING (vkimg.h)

#ifdef VK_QC_NSTAT
static_assert(kQcNstat == VK_QC_NSTAT && kQcQualAt == VK_QC_QUAL_HIST && kQcReadqAt == VK_QC_READQ_HIST && kQcLenAt == VK_QC_LEN_HIST &&
              kQcBaseAt == VK_QC_CYCLE_BASE && kQcQsumAt == VK_QC_CYCLE_QSUM && kQcCycles == VK_QC_CYCLES &&
              kQcBadFraming == VK_QC_BAD_FRAMING, "the row of include/vkimg.h");
#endif
static_assert(kQcMerge >= 1 && kQcMerge < (1u << (32 - kQcSumBits)), "a cycle cell counts a workgroup's records in 10 bits");
static_assert(93ull * kQcMerge < (1ull << kQcSumBits), "a cycle cell sums a workgroup's qualities in 22 bits");

struct QcTile {   // a workgroup's private counters
    uint32_t cyc[kQcClasses * kQcCycles];   // [class][cycle]: lanes on consecutive cycles, consecutive banks
    uint32_t qual[kQcPhreds * kQcCopies];   // [phred][copy]
    uint32_t len[kQcLenBins];
    uint32_t readq[kQcPhreds];
    uint32_t maxc;                          // cycles in use
};

struct QcLane {   // a lane's sums
    uint32_t gc = 0, other = 0, invalid = 0;   // over the workgroup's records (a stream is shorter than 2^32 bytes)
    uint64_t qsum = 0;                         // over one record
};

// A0 C1 G2 T3 in either case; 4: every other byte.  Without a branch (written as a chain of comparisons hipcc made it a
// tree of divergent branches per base): with the case bit dropped, A C G T are 0, 2, 6 and 19 past 'A', a bit each of a
// mask; bits 1..2 of the byte are 0 1 3 2 for A C G T, and c ^ (c >> 1) puts G and T in order.
__device__ inline uint32_t qc_class(uint32_t b) {
    const uint32_t u = (b & 0xDFu) - 'A';
    const uint32_t is_base = (0x80045u >> (u & 31u)) & (u < 32u ? 1u : 0u);
    const uint32_t c = (b >> 1) & 3u;
    return is_base ? c ^ (c >> 1) : 4u;
}

__device__ inline uint32_t qc_phred(uint32_t b, uint32_t* invalid) {   // byte - 33 clamped to 0..93
    *invalid = b < 33u || b > 126u ? 1u : 0u;
    return b < 33u ? 0u : b > 126u ? 93u : b - 33u;
}

// A lane's share of the cycles [c0, c0 + kQcChunk) of a record of ls bases: cycles c0 + lane, + 64, + 128, + 192, each
// read once (the loads first, then the counting).
__device__ inline void qc_lane_chunk(const uint8_t* seq, const uint8_t* qual, uint64_t c0, uint64_t ls, uint32_t lane, QcTile* T,
                                     QcLane* a) {
    uint32_t sb[kQcChunk / 64], qb[kQcChunk / 64];
    for (uint32_t i = 0; i < kQcChunk / 64; ++i) {
        const uint64_t c = c0 + 64u * i + lane;
        sb[i] = qb[i] = 0;
        if (c < ls) {
            sb[i] = seq[c];
            qb[i] = qual[c];
        }
    }
    for (uint32_t i = 0; i < kQcChunk / 64; ++i) {
        const uint64_t c = c0 + 64u * i + lane;
        if (c >= ls) continue;
        uint32_t bad;
        const uint32_t cls = qc_class(sb[i]), q = qc_phred(qb[i], &bad);
        a->gc += cls == 1u || cls == 2u ? 1u : 0u;
        a->other += cls == 4u ? 1u : 0u;
        a->invalid += bad;
        a->qsum += q;
        QC_ADD32(&T->qual[q * kQcCopies + (lane & (kQcCopies - 1u))], 1u);
        if (c < kQcCycles) QC_ADD32(&T->cyc[cls * kQcCycles + static_cast<uint32_t>(c)], (1u << kQcSumBits) | q);
    }
}

// The merge, thread t of n: every cell of the tile that holds something goes to the row.
__device__ inline void qc_merge(const QcTile* T, uint64_t* row, uint32_t t, uint32_t n) {
    const uint32_t maxc = T->maxc < kQcCycles ? T->maxc : kQcCycles;
    for (uint32_t i = t; i < kQcClasses * maxc; i += n) {
        const uint32_t c = i / kQcClasses, cls = i % kQcClasses;
        const uint32_t v = T->cyc[cls * kQcCycles + c];
        if (v >> kQcSumBits) QC_ADD64(row + kQcBaseAt + i, static_cast<uint64_t>(v >> kQcSumBits));
        if (v & ((1u << kQcSumBits) - 1u)) QC_ADD64(row + kQcQsumAt + i, static_cast<uint64_t>(v & ((1u << kQcSumBits) - 1u)));
    }
    for (uint32_t q = t; q < kQcPhreds; q += n) {
        uint64_t v = 0;
        // (copy (j + q) % 32 first: the lanes of a group start on different banks)
        for (uint32_t j = 0; j < kQcCopies; ++j) v += T->qual[q * kQcCopies + ((j + q) & (kQcCopies - 1u))];
        if (v) QC_ADD64(row + kQcQualAt + q, v);
        if (T->readq[q]) QC_ADD64(row + kQcReadqAt + q, static_cast<uint64_t>(T->readq[q]));
    }
    for (uint32_t i = t; i < kQcLenBins; i += n)
        if (T->len[i]) QC_ADD64(row + kQcLenAt + i, static_cast<uint64_t>(T->len[i]));
}

#ifndef VK_QC_LANE_ONLY

using QcStream = EmSample;   // a stream is a sample of the record index: its text, its budgeted records, its chunks (vk_emit.h)

__global__ void __launch_bounds__(kClThreads) vk_qc_status_kernel(const uint8_t* text, const QcStream* streams, uint32_t nstreams,
                                                                 const uint64_t* nl_prefix, uint64_t* rows, uint32_t* status) {
    const uint32_t si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= nstreams) return;
    const QcStream s = streams[si];
    uint64_t lines = 0;
    if (s.len) lines = nl_prefix[s.chunk1] - nl_prefix[s.chunk0] + (text[s.off + s.len - 1] != '\n' ? 1u : 0u);
    status[si] = lines < 4 * s.nrec ? kEmBadRecords : 0u;
    rows[static_cast<uint64_t>(si) * kQcNstat + kQcMinLen] = ~0ull;   // (the smallest length is taken with atomicMin)
}

__device__ inline uint32_t qc_uniform(uint32_t v) {   // a value that every lane of the wave holds, as a scalar
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

__device__ inline uint32_t qc_lane_value(uint32_t v, uint32_t lane) {   // lane `lane`'s v, as a scalar
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(lane)));
}

template <class T>
__device__ inline T qc_wave_sum(T v) {
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_down(v, d, 64);
    return v;   // (lane 0's)
}

__global__ void __launch_bounds__(kQcThreads) vk_qc_count_kernel(const uint8_t* text, const QcStream* streams,
                                                                const uint64_t* block_base, uint32_t nstreams, uint32_t per_block,
                                                                const ClRec* recs, uint64_t* rows, const uint32_t* status,
                                                                uint32_t* bad_framing) {
    __shared__ QcTile T;
    const uint32_t si = cl_find_u64(block_base, nstreams, blockIdx.x);
    if (status[si] != 0) return;   // (VK_EM_BAD_RECORDS: records without their line ends; the workgroup's one answer)
    const QcStream s = streams[si];
    for (uint32_t i = threadIdx.x; i < sizeof(QcTile) / 4; i += kQcThreads) reinterpret_cast<uint32_t*>(&T)[i] = 0;
    __syncthreads();
    const uint32_t wave = qc_uniform(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint64_t r0 = (blockIdx.x - block_base[si]) * per_block;
    const uint32_t n = static_cast<uint32_t>(min(static_cast<uint64_t>(per_block), s.nrec - r0));
    QcLane a;
    // the wave's own sums (every lane holds them)
    uint64_t n_rec = 0, n_ragged = 0, bases = 0;
    uint32_t lmin = ~0u, lmax = 0;
    bool bad = false;
    // A record costs three trips to memory, one behind the other: its line ends (fetched while the record before is
    // counted), its four framing bytes (a lane each, one load), its sequence and quality bytes.
    const ClRec* rp = recs + s.rec0 + r0;
    const uint64_t end = s.off + s.len;
    ClRec r = rp[wave < n ? wave : 0u], nxt;
    for (uint32_t j = wave; j < n; j += kQcThreads / 64, r = nxt) {
        const uint32_t jn = j + kQcThreads / 64;
        nxt = rp[jn < n ? jn : j];
        const uint64_t qe = r.qe == ~0ull ? end : r.qe;   // (the stream's last line may lack its newline)
        // the header's first byte, the third line's (r.se + 1 <= r.pe: its first byte or its newline), and the last bytes
        // of the sequence and quality lines (of an empty line: the newline in front of it)
        const uint64_t at = lane == 0 ? r.h : lane == 1 ? r.se + 1 : lane == 2 ? r.se - 1 : qe - 1;
        const uint32_t fb = lane < 4 ? text[at] : 0u;
        if (qc_lane_value(fb, 0) != '@' || qc_lane_value(fb, 1) != '+') {
            bad = true;
            break;
        }
        const uint64_t sq = r.he + 1, qq = r.pe + 1;
        uint32_t L = static_cast<uint32_t>(r.se - sq), Lq = static_cast<uint32_t>(qe - qq);
        if (L && qc_lane_value(fb, 2) == '\r') --L;
        if (Lq && qc_lane_value(fb, 3) == '\r') --Lq;
        ++n_rec;
        if (L != Lq) {
            ++n_ragged;
            continue;
        }
        const uint32_t ls = qc_uniform(L);
        a.qsum = 0;
        for (uint64_t c0 = 0; c0 < ls; c0 += kQcChunk) qc_lane_chunk(text + sq, text + qq, c0, ls, lane, &T, &a);
        // (a read of fewer than 2^25 bases: its qualities sum to less than 2^32, and 32-bit sums and a 32-bit division do)
        const bool narrow = ls < (1u << 25);
        const uint64_t qsum = narrow ? qc_wave_sum(static_cast<uint32_t>(a.qsum)) : qc_wave_sum(a.qsum);
        bases += ls;
        lmin = min(lmin, ls);
        lmax = max(lmax, ls);
        if (lane == 0) {
            atomicAdd(&T.len[min(ls, kQcLenBins - 1u)], 1u);
            if (ls) atomicAdd(&T.readq[narrow ? static_cast<uint32_t>(qsum) / ls : static_cast<uint32_t>(qsum / ls)], 1u);
        }
    }
    const uint64_t gc = qc_wave_sum(static_cast<uint64_t>(a.gc)), other = qc_wave_sum(static_cast<uint64_t>(a.other)),
                   invalid = qc_wave_sum(static_cast<uint64_t>(a.invalid));
    if (lane == 0) {
        if (bad) atomicOr(bad_framing + si, 1u);
        atomicMax(&T.maxc, min(lmax, kQcCycles));
        // (the scalars: a handful of additions per wavefront and workgroup, straight to the row)
        unsigned long long* row = reinterpret_cast<unsigned long long*>(rows + static_cast<uint64_t>(si) * kQcNstat);
        if (n_rec) atomicAdd(row + kQcRecords, static_cast<unsigned long long>(n_rec));
        if (n_ragged) atomicAdd(row + kQcRagged, static_cast<unsigned long long>(n_ragged));
        if (bases) atomicAdd(row + kQcBases, static_cast<unsigned long long>(bases));
        if (gc) atomicAdd(row + kQcGc, static_cast<unsigned long long>(gc));
        if (other) atomicAdd(row + kQcOther, static_cast<unsigned long long>(other));
        if (invalid) atomicAdd(row + kQcInvalid, static_cast<unsigned long long>(invalid));
        if (n_rec > n_ragged) {
            atomicMin(row + kQcMinLen, static_cast<unsigned long long>(lmin));
            atomicMax(row + kQcMaxLen, static_cast<unsigned long long>(lmax));
        }
    }
    __syncthreads();
    qc_merge(&T, rows + static_cast<uint64_t>(si) * kQcNstat, threadIdx.x, kQcThreads);
}

__global__ void __launch_bounds__(kClThreads) vk_qc_finish_kernel(uint64_t* rows, uint32_t* status, const uint32_t* bad_framing) {
    uint64_t* row = rows + static_cast<uint64_t>(blockIdx.x) * kQcNstat;
    const uint32_t st = status[blockIdx.x] | (bad_framing[blockIdx.x] ? kQcBadFraming : 0u);   // (every thread reads before one writes)
    __syncthreads();
    if (st != 0) {
        for (uint32_t i = threadIdx.x; i < kQcNstat; i += kClThreads) row[i] = 0;
        if (threadIdx.x == 0) status[blockIdx.x] = st;
    } else if (threadIdx.x == 0 && row[kQcMinLen] == ~0ull) {
        row[kQcMinLen] = 0;
    }
}

#endif  // VK_QC_LANE_ONLY

}  // namespace

#endif  // VK_QC_H
