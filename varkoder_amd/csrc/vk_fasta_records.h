// vk_fasta_records.h -- one histogram per FASTA RECORD: `image / query --from-fasta --per-record`
// (vk_fasta_records_count_device, vk_fasta_records_device, vk_count_fasta_records_device).  Part of the one translation
// unit vkimg.hip, on top of vk_fasta.h: the same cut by bytes (lanes of kFaLaneBytes, units, spans of units), the same
// rule for lines, headers and bases, the same walk (FaWalk).
//
// The rule ("--from-fasta --per-record"; tests/fasta_records_ref.py is the same rule in Python): a sample
// that starts with '>' has one record per header line, ordinals 0 .. nrec - 1; record r has a start (the offset of its
// '>'), bases (its joined bytes, every class), a name (its header line behind the '>', at most kFaNameBytes kept) and the
// histogram vk_count_fasta_device gives for a sample that holds this record alone.  The caller names a row (slot) per
// record, or kFaNoSlot: such a record is not counted.
//
// The text is still cut by bytes: a record may be a chromosome or 300 bases, and a lane of 64 bytes may hold 32 of them.
//   * Record ordinal.  The record of a byte is (header line starts up to and including it) - 1.  Every lane states how
//     many header lines start in its bytes; an exclusive SUM over the lanes of the unit, beside vk_fasta.h's exclusive
//     maximum and in the same shuffles and barriers (fa_block_excl_max_sum), and over the units of the sample
//     (vk_far_scan_kernel, with a running carry over its passes) give every lane the count before its first byte.
//         vk_far_summary_kernel   per unit: vk_fasta.h's pair and the header lines that start in it
//         vk_far_scan_kernel      workgroup per sample: header state and header count that enter every unit; status; nrec
//         vk_far_table_kernel     start, bases and name of every record
//         vk_far_count_kernel<K>  the count
//   * Table.  The lane that holds a record's '>' writes its start and copies its name, reading on across whatever seam as
//     the tail walk does.  Every lane adds the sequence bytes it owns to the record they fall in, one atomic per record.
//   * Count.  FaWalk, unchanged.  At a header line start among its own bytes a lane flushes its pending addition, steps
//     the ordinal and looks the next row up; the tail walk behind its own bytes stops at a header line as before, so its
//     windows belong to the record current when the own bytes ended.
//     k <= 7: the workgroup's LDS table belongs to the record that ENTERS its span (at the sample's first span: record
//     0).  Windows of any other record go to their row with global atomics.  The table is flushed to the entering
//     record's row at the end, and is neither zeroed nor used when that record has no slot.  A chromosome keeps every
//     workgroup but its first on ds_add_u32; many short records land on many rows, where global atomics do not contend.
//     k = 8, 9: global atomics on the rows.  A wave all of whose lanes are whole, in the entering record and without a
//     header line start runs vk_fa_count_kernel's unrolled loop; any other wave runs a rolled loop with the header test.
//   * Skipping.  A workgroup none of whose records has a slot returns before it loads any text: a call's slots are
//     consecutive records of a batch, most workgroups lie outside them.
// Ordinals and slots from the caller are bounds-checked on the device: a record past rec_first's count, or a slot of
// nslots or more, has no row.
// The lane-local code (fa_lane_headers, far_lane_table, far_lane_count) compiles for the host:
// tests/emul/fasta_records_emul.cpp.
#ifndef VK_FASTA_RECORDS_H
#define VK_FASTA_RECORDS_H

#include "vk_fasta.h"

namespace {

constexpr uint32_t kFaNameBytes = 128;        // VK_FA_NAME_BYTES
constexpr uint32_t kFaNoSlot = 0xFFFFFFFFu;   // VK_FA_NO_SLOT

// 0x80 in every byte of x that equals the byte pat repeats (exact: no carry leaves a byte).
__device__ inline uint32_t fa_eq_mask(uint32_t x, uint32_t pat) {
    const uint32_t y = x ^ pat;
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}

// Header lines that start among a lane's n bytes (first_ls: its first byte starts a line).  Word arithmetic, no byte
// loop: a '>' counts where the byte before it is a '\n'.
__device__ inline uint32_t fa_lane_headers(const uint32_t* w, uint32_t n, bool first_ls) {
    // Sequence text holds no '>' at all: a test of the words (it may give a false alarm, never miss one; bytes past n
    // take part) spares nearly every lane of an assembly the rest.
    uint32_t any = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFaLaneBytes / 4; ++j) {
        const uint32_t y = w[j] ^ 0x3E3E3E3Eu;
        any |= (y - 0x01010101u) & ~y;
    }
    if (!(any & 0x80808080u)) return 0;
    uint32_t nh = 0, carry = first_ls ? 0x80u : 0u;   // (the line end before a word's first byte)
#pragma unroll
    for (uint32_t j = 0; j < kFaLaneBytes / 4; ++j) {
        const uint32_t keep = n >= 4 * j + 4 ? 0xFFFFFFFFu : n <= 4 * j ? 0u : (1u << (8 * (n - 4 * j))) - 1u;   // bytes past n: 0
        const uint32_t x = w[j] & keep;
        const uint32_t nl = fa_eq_mask(x, 0x0A0A0A0Au);
        const uint32_t hit = fa_eq_mask(x, 0x3E3E3E3Eu) & ((nl << 8) | carry);
        nh += ((hit >> 7) * 0x01010101u) >> 24;
        carry = nl >> 24;
    }
    return nh;
}

// The two walks below go over a lane's words in a ROLLED loop of sixteen trips, four bytes each, and hand the words down
// a register at a time (x[0] is the current one): what they do at a header line start -- atomics, a table lookup, the
// copy of a name -- would otherwise stand sixty-four times in the kernel, each under a mask of its own.

// A lane's part of the record table.  hdr, first_ls: the state at its first byte; next: the byte behind its last one,
// '\n' at the sample's end (a '\r' before a line end or as the last byte is no sequence); hb: header lines that start
// before its first byte.  sink.header(ordinal, i): record `ordinal` starts at the lane's byte i; sink.bases(ordinal, nb):
// nb sequence bytes of the lane belong to that record (ordinal = 0xFFFFFFFF: bytes before any header, a bad start).
template <class Sink>
__device__ inline void far_lane_table(const uint32_t* w, uint32_t n, uint32_t hdr, bool first_ls, uint32_t next, uint32_t hb, Sink& sink) {
    uint32_t x[kFaLaneBytes / 4];
#pragma unroll
    for (uint32_t q = 0; q < kFaLaneBytes / 4; ++q) x[q] = w[q];
    uint32_t nb = 0;
    bool ls = first_ls;
#pragma unroll 1
    for (uint32_t j = 0; j < kFaLaneBytes / 4; ++j) {
        const uint32_t v = x[0], behind = x[1];
#pragma unroll
        for (uint32_t q = 0; q + 1 < kFaLaneBytes / 4; ++q) x[q] = x[q + 1];
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const uint32_t i = 4 * j + t;
            if (i < n) {
                const uint32_t b = (v >> (8 * t)) & 255u;
                const uint32_t nx = i + 1 < n ? (t < 3 ? (v >> (8 * ((t + 1) & 3u))) & 255u : behind & 255u) : next;
                if (ls && b == '>') {
                    if (nb) sink.bases(hb - 1u, nb);
                    nb = 0;
                    sink.header(hb, i);
                    ++hb;
                }
                hdr = ls ? (b == '>' ? 1u : 0u) : hdr;
                ls = b == '\n';
                nb += !ls && !hdr && !(b == '\r' && nx == '\n') ? 1u : 0u;
            }
        }
    }
    if (nb) sink.bases(hb - 1u, nb);
}

// A lane's own bytes of the count: FaWalk's steps, and at a header line start the pending addition goes to the row it
// was made for before add.enter(ordinal) names the next one.  hb: header lines that start before the lane's first byte;
// returns the same behind its last.
template <int K, class Add>
__device__ inline uint32_t far_lane_count(const uint32_t* w, uint32_t n, FaWalk& wk, uint32_t hb, Add& add) {
    uint32_t x[kFaLaneBytes / 4];
#pragma unroll
    for (uint32_t q = 0; q < kFaLaneBytes / 4; ++q) x[q] = w[q];
#pragma unroll 1
    for (uint32_t j = 0; j < kFaLaneBytes / 4; ++j) {
        const uint32_t v = x[0];
#pragma unroll
        for (uint32_t q = 0; q + 1 < kFaLaneBytes / 4; ++q) x[q] = x[q + 1];
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            if (4 * j + t < n) {
                const uint32_t b = (v >> (8 * t)) & 255u;
                if (wk.ls && b == '>') {
                    wk.flush(add);
                    add.enter(hb);
                    ++hb;
                }
                wk.template step<K>(b, true, add);
            }
        }
    }
    return hb;
}

#ifndef VK_FASTA_LANE_ONLY

// fa_block_excl_max of `key` and, in the same shuffles and barriers, the exclusive sum of `cnt` over the lanes of the
// workgroup in lane order (all kFaThreads lanes call it).  s_wave: 2 * (kFaThreads / 64) words of LDS.
__device__ inline uint32_t fa_block_excl_max_sum(uint32_t key, uint32_t cnt, uint32_t* s_wave, uint32_t* key_total, uint32_t* excl_sum,
                                                 uint32_t* sum_total) {
    constexpr uint32_t NW = kFaThreads / 64;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = key, sum = cnt;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        const uint32_t a = __shfl_up(sum, d, 64);
        if (lane >= d && o > inc) inc = o;
        if (lane >= d) sum += a;
    }
    if (lane == 63) {
        s_wave[wave] = inc;
        s_wave[NW + wave] = sum;
    }
    uint32_t excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 0;
    uint32_t before = sum - cnt;
    __syncthreads();
    uint32_t all = 0, all_sum = 0;
#pragma unroll
    for (uint32_t v = 0; v < NW; ++v) {
        const uint32_t t = s_wave[v], c = s_wave[NW + v];
        if (v < wave && t > excl) excl = t;
        if (v < wave) before += c;
        if (t > all) all = t;
        all_sum += c;
    }
    __syncthreads();   // (s_wave is written again by the next call)
    *key_total = all;
    *excl_sum = before;
    *sum_total = all_sum;
    return excl;
}

// The records of a batch as the caller knows them.
struct FaRecs {
    const uint64_t* rec_first;   // [nsamples + 1] device: the first record of each sample in the batch's tables
};

__global__ __launch_bounds__(kFaThreads) void vk_far_summary_kernel(const uint8_t* base, FaMeta m, uint32_t* ukey, uint32_t* uhdr) {
    __shared__ uint32_t s_wave[2 * (kFaThreads / 64)];
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
        const uint32_t nh = fa_lane_headers(w, n, first_ls);
        uint32_t total, before, headers;
        (void)fa_block_excl_max_sum(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, nh, s_wave, &total, &before, &headers);
        if (threadIdx.x == 0) {
            ukey[m.unit_first[s] + u] = total ? 2u | (total & 1u) : 0u;
            uhdr[m.unit_first[s] + u] = headers;
        }
    }
}

// carry[unit]: the header state that enters it (vk_fa_scan_kernel's); uhdr[unit]: in, the header lines that start in it;
// out, those that start before it.  nrec[s]: the sample's records (0 with VK_ST_BAD_START).
__global__ __launch_bounds__(kFaThreads) void vk_far_scan_kernel(const uint8_t* base, FaMeta m, const uint32_t* ukey, uint32_t* carry,
                                                                 uint32_t* uhdr, uint32_t* status, uint32_t* nrec) {
    __shared__ uint32_t s_wave[2 * (kFaThreads / 64)];
    const uint32_t s = blockIdx.x;
    const uint64_t first = m.unit_first[s], nunits = m.unit_first[s + 1] - first;   // (nunits < 2^30: the caller checks)
    uint32_t running = 0, running_sum = 0;
    for (uint64_t t = 0; t < nunits; t += kFaThreads) {
        const uint64_t u = t + threadIdx.x;
        const uint32_t k = u < nunits ? ukey[first + u] : 0u;
        const uint32_t c = u < nunits ? uhdr[first + u] : 0u;
        uint32_t total, before, headers;
        uint32_t excl = fa_block_excl_max_sum(k ? (static_cast<uint32_t>(u + 1) << 1) | (k & 1u) : 0u, c, s_wave, &total, &before, &headers);
        if (running > excl) excl = running;
        if (u < nunits) {
            carry[first + u] = excl & 1u;   // (nothing before: not in a header line)
            uhdr[first + u] = running_sum + before;
        }
        if (total > running) running = total;
        running_sum += headers;
    }
    if (threadIdx.x == 0) {
        const bool bad = m.lens[s] && base[m.offs[s]] != '>';
        status[s] = bad ? 1u : 0u;   // VK_ST_BAD_START
        nrec[s] = bad ? 0u : running_sum;
    }
}

struct FarTableSink {
    const uint8_t* text;
    uint64_t len, c0, g0;   // the lane's first byte; the sample's first record in the tables
    uint32_t nrec;          // the sample's records as the caller counts them: nothing is written past them
    unsigned long long* rec_start;
    unsigned long long* rec_bases;
    uint8_t* rec_name;
    __device__ inline void header(uint32_t ord, uint32_t i) {
        if (ord >= nrec) return;
        rec_start[g0 + ord] = c0 + i;
        uint8_t* name = rec_name + (g0 + ord) * kFaNameBytes;
        uint64_t p = c0 + i + 1;
        for (uint32_t j = 0; j < kFaNameBytes && p < len; ++j, ++p) {
            const uint8_t b = text[p];
            if (b == '\n') break;
            name[j] = b;
        }
    }
    __device__ inline void bases(uint32_t ord, uint32_t nb) {
        if (ord < nrec) atomicAdd(rec_bases + g0 + ord, static_cast<unsigned long long>(nb));
    }
};

// rec_start, rec_bases and rec_name come in zeroed.
__global__ __launch_bounds__(kFaThreads) void vk_far_table_kernel(const uint8_t* base, FaMeta m, const uint32_t* carry, const uint32_t* uhdr,
                                                                  FaRecs rc, unsigned long long* rec_start, unsigned long long* rec_bases,
                                                                  uint8_t* rec_name) {
    __shared__ uint32_t s_wave[2 * (kFaThreads / 64)];
    uint64_t u0, u1;
    const uint32_t s = fa_locate(m, blockIdx.x, &u0, &u1);
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    if (text[0] != '>') return;   // VK_ST_BAD_START (a sample with a workgroup is not empty): no records
    const uint64_t g0 = rc.rec_first[s], gn = rc.rec_first[s + 1] - g0;
    const uint32_t nrec = gn < 0xFFFFFFFFull ? static_cast<uint32_t>(gn) : 0xFFFFFFFEu;
    for (uint64_t u = u0; u < u1; ++u) {
        uint32_t w[kFaLaneBytes / 4], n;
        uint64_t c0;
        fa_load(text, len, u, m.unit_bytes, w, &c0, &n);
        const bool first_ls = n && (c0 == 0 || text[c0 - 1] == '\n');
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        const uint32_t nh = fa_lane_headers(w, n, first_ls);
        uint32_t total, before, headers;
        const uint32_t excl = fa_block_excl_max_sum(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, nh, s_wave, &total, &before, &headers);
        if (n == 0) continue;   // (uniform calls above; nothing below meets a barrier)
        const uint64_t unit = m.unit_first[s] + u;
        const uint32_t hdr = excl ? excl & 1u : carry[unit];
        const uint32_t next = c0 + n < len ? text[c0 + n] : '\n';
        FarTableSink sink{text, len, c0, g0, nrec, rec_start, rec_bases, rec_name};
        far_lane_table(w, n, hdr, first_ls, next, uhdr[unit] + before, sink);
    }
}

// Where a lane's additions go: the workgroup's LDS table while it is in the record that table belongs to, else the row of
// its record, else nowhere.
template <int K>
struct FarAdd {
    static constexpr uint32_t NCODE = 1u << (2 * K);
    uint32_t* s_hist;          // the workgroup's LDS table (K <= 7)
    uint32_t* hist;
    const uint32_t* slot;      // of the sample's records
    uint32_t nrec, nslots;
    uint32_t own;              // the record the LDS table belongs to; kFaNoSlot: none (K = 8, 9, or that record has no slot)
    bool to_lds = false;
    uint32_t* row = nullptr;

    __device__ inline void enter(uint32_t ord) {
        to_lds = ord == own;
        row = nullptr;
        if (to_lds || ord >= nrec) return;
        const uint32_t sl = slot[ord];
        if (sl < nslots) row = hist + static_cast<size_t>(sl) * NCODE;
    }
    __device__ inline bool any() const { return to_lds || row; }
    __device__ inline void operator()(uint32_t code, uint32_t n) {
        if (to_lds) atomicAdd(s_hist + code, n);
        else if (row) atomicAdd(row + code, n);
    }
};

template <int K>
__global__ __launch_bounds__(kFaThreads) void vk_far_count_kernel(const uint8_t* base, FaMeta m, const uint32_t* carry, const uint32_t* uhdr,
                                                                  const uint32_t* nrec_seen, FaRecs rc, const uint32_t* slot, uint32_t nslots,
                                                                  uint32_t* hist) {
    constexpr uint32_t NCODE = 1u << (2 * K);
    constexpr bool LDSH = K <= 7;
    __shared__ uint32_t s_hist[LDSH ? NCODE : 1];
    __shared__ uint32_t s_wave[2 * (kFaThreads / 64)];
    uint64_t u0, u1;
    const uint32_t s = fa_locate(m, blockIdx.x, &u0, &u1);
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    if (text[0] != '>') return;   // VK_ST_BAD_START (a sample with a workgroup is not empty): no records
    const uint64_t first = m.unit_first[s], nunits = m.unit_first[s + 1] - first;
    const uint64_t g0 = rc.rec_first[s], gn = rc.rec_first[s + 1] - g0;
    const uint32_t nrec = gn < 0xFFFFFFFFull ? static_cast<uint32_t>(gn) : 0xFFFFFFFEu;
    const uint32_t* sslot = slot + g0;
    // the records of this span: the one that enters it up to the last one that starts in it
    const uint32_t hb0 = uhdr[first + u0];
    const uint32_t hb1 = u1 < nunits ? uhdr[first + u1] : nrec_seen[s];
    const uint32_t own_ord = hb0 ? hb0 - 1u : 0u;
    uint32_t last = hb1 ? hb1 - 1u : 0u;
    if (last >= nrec) last = nrec ? nrec - 1u : 0u;
    int mine = 0;
    for (uint64_t r = static_cast<uint64_t>(own_ord) + threadIdx.x; r <= last && r < nrec; r += kFaThreads) mine |= sslot[r] < nslots ? 1 : 0;
    if (!__syncthreads_or(mine)) return;   // (uniform) none of them has a slot: the text is not read
    const uint32_t own_slot = own_ord < nrec ? sslot[own_ord] : kFaNoSlot;
    const bool lds_on = LDSH && own_slot < nslots;
    if (lds_on) {
        for (uint32_t i = threadIdx.x; i < NCODE; i += kFaThreads) s_hist[i] = 0;
        __syncthreads();
    }
    for (uint64_t u = u0; u < u1; ++u) {
        uint32_t w[kFaLaneBytes / 4], n;
        uint64_t c0;
        fa_load(text, len, u, m.unit_bytes, w, &c0, &n);
        const bool first_ls = n && (c0 == 0 || text[c0 - 1] == '\n');
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        const uint32_t nh = fa_lane_headers(w, n, first_ls);
        uint32_t total, before, headers;
        const uint32_t excl = fa_block_excl_max_sum(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, nh, s_wave, &total, &before, &headers);
        if (n == 0) continue;   // (uniform calls above; nothing below meets a barrier)
        const uint32_t hb = uhdr[first + u] + before;   // header lines that start before this lane
        FaWalk wk;
        wk.hdr = excl ? excl & 1u : carry[first + u];
        wk.ls = first_ls ? 1u : 0u;
        // (lanes that left at n == 0 are not in the vote: only a wave's active lanes are asked)
        const bool plain = !__any(nh != 0 || hb != own_ord + 1u || n != kFaLaneBytes);
        if (plain) {
            // the whole wave lies in the entering record, holds no header line start and no lane of it is cut short by
            // the sample's end: vk_fa_count_kernel's loop, without its test of the lane's length
            if (own_slot >= nslots) continue;
            FaAdd<K> add{LDSH ? s_hist : hist + static_cast<size_t>(own_slot) * NCODE};
#pragma unroll
            for (uint32_t i = 0; i < kFaLaneBytes; ++i) wk.template step<K>(fa_byte(w, i), true, add);
            for (uint64_t p = c0 + n; p < len && wk.template more<K>(); ++p) wk.template step<K>(text[p], false, add);
            wk.flush(add);
            continue;
        }
        FarAdd<K> add{s_hist, hist, sslot, nrec, nslots, lds_on ? own_ord : kFaNoSlot};
        if (hb) add.enter(hb - 1u);
        if (nh == 0 && !add.any()) continue;   // in a record without a row, and no other begins here
        (void)far_lane_count<K>(w, n, wk, hb, add);
        for (uint64_t p = c0 + n; p < len && wk.template more<K>(); ++p) wk.template step<K>(text[p], false, add);
        wk.flush(add);
    }
    if (lds_on) {
        __syncthreads();
        uint32_t* row = hist + static_cast<size_t>(own_slot) * NCODE;
        for (uint32_t i = threadIdx.x; i < NCODE; i += kFaThreads) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(row + i, v);
        }
    }
}

#endif  // VK_FASTA_LANE_ONLY

}  // namespace

#endif  // VK_FASTA_RECORDS_H
