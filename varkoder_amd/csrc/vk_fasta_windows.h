// vk_fasta_windows.h -- one histogram per WINDOW of a FASTA record: `image / query --from-fasta --windows`
// (vk_count_fasta_windows_device).  Part of the one translation unit vkimg.hip, on top of vk_fasta.h (the cut by bytes,
// FaWalk), vk_fasta_records.h (the record ordinal of every lane, the switch of the target row at a header line) and
// vk_fasta_ladder.h (the index of sequence-byte ordinals); their kernels run unchanged in front of the two below.
//
// The rule ("--from-fasta --windows"; tests/fasta_windows_ref.py is the same rule in Python): a call has
// a window length N and a step S, S | N, m = N / S <= 64.  Window w of a record covers its ordinals [wS, wS + N) and
// exists iff it lies in the record; its histogram holds the record's counted k-mers whose FIRST byte lies in it.  A
// record has a first row win_first (or kFaNoWindow), window w has row win_first + w, and a call counts the rows of
// [row_lo, row_lo + nrows).
//
// TILES.  Tile t of a record holds the k-mers that start in [tS, tS + S); window w is the sum of the tiles w .. w + m - 1,
// exactly (assignment is by start, so no k-mer belongs to two tiles or to none).  The text is read once whatever m is:
//   vk_faw_plan_kernel     one workgroup over the records of the batch: where the joined bytes of every record start
//                          (an exclusive sum of rec_bases), which of its tiles the call needs and the row of the first
//                          of them: a row of d_hist when m = 1, a row of the tile workspace (an exclusive sum of the
//                          tiles needed) when m > 1.  Everything the caller states is clipped here: a record's rows
//                          to the range, the tile rows to the workspace.
//   vk_faw_count_kernel<K> the count of tiles
//   vk_faw_sum_kernel      m > 1: every window row of the range = the sum of its m tile rows (plain stores; no atomics)
//   * A lane knows at its first byte: the record (header lines that start before it, vk_far_scan_kernel), the ordinal
//     of its first sequence byte in the sample (the ladder's index) and so in the record, and from that the tile and
//     the offset in it of the k-mer the next sequence byte would complete (FawPos: that k-mer starts K - 1 bytes back).
//   * The row changes inside a lane at a tile seam and at a header line; the pending addition is flushed before either.
//     The tail walk behind a lane's own bytes keeps stepping the position, so a k-mer that starts in the lane's last
//     bytes goes to the tile of its start wherever it completes.
//   * k <= 7: the workgroup's LDS table belongs to the (record, tile) that ENTERS its span.  Tiles of a few thousand
//     bases are much shorter than a span, and a tile shorter than 4^k bases gains nothing from a table of its own (its
//     flush would be as many global atomics as its k-mers), so every other tile goes to its row with global atomics,
//     which land on many rows and do not contend.  The table pays where S is large: then most workgroups lie in one
//     tile.  k = 8, 9: global atomics on the rows.
//   * A wave whose lanes are whole, hold no header line start and no seam and lie in one tile runs vk_fa_count_kernel's
//     unrolled loop on that tile's row (or the LDS table); any other wave runs the rolled loop.
//   * Skipping.  A workgroup none of whose bytes can map to a needed tile returns before it loads text; a lane of a
//     record without a header line start whose tiles are not needed is not walked.
// Ordinals, win_first and row numbers come from the caller and are bounds-checked on the device: a record past
// rec_first's count, a tile outside the needed ones or a row outside its buffer has no row.
// The lane-local code (FawPos, faw_step, faw_lane_count) compiles for the host: tests/emul/fasta_windows_emul.cpp.
#ifndef VK_FASTA_WINDOWS_H
#define VK_FASTA_WINDOWS_H

#include "vk_fasta_ladder.h"
#include "vk_fasta_records.h"

namespace {

constexpr uint64_t kFaNoWindow = 0xFFFFFFFFFFFFFFFFull;   // VK_FA_NO_WINDOW
constexpr uint32_t kFaMaxSteps = 64;                      // m = N / S
constexpr uint32_t kFawSumCodes = 1024;   // codes of a row a workgroup of the sum handles (4^5: every k has whole chunks)

// Where the k-mer that the NEXT sequence byte of a record would complete starts: its tile and the offset in it.  A
// record's first K - 1 bytes complete nothing: there the offset is negative and the tile 0.
struct FawPos {
    uint64_t tile = 0;
    int32_t r = 0;      // -(K - 1) .. S - 1
    uint32_t S = 1;

    // rel: the record ordinal of the next sequence byte
    template <int K>
    __device__ inline void start(uint64_t rel, uint32_t step) {
        S = step;
        if (rel < static_cast<uint64_t>(K - 1)) {
            tile = 0;
            r = static_cast<int32_t>(rel) - (K - 1);
        } else {
            const uint64_t p = rel - (K - 1);
            tile = p / S;
            r = static_cast<int32_t>(p - tile * S);
        }
    }
    // a sequence byte has been taken; true: the next k-mer starts in another tile
    __device__ inline bool advance() {
        if (++r != static_cast<int32_t>(S)) return false;
        r = 0;
        ++tile;
        return true;
    }
};

// FaWalk's step with the position kept: what the byte completes goes to the tile named before it; behind a sequence byte
// (a '\r' is one only once the byte behind it is no '\n') the position moves on, and at a seam the pending addition goes
// to the row it was made for before add.tile() names the next one.
template <int K, class Add>
__device__ inline void faw_step(FaWalk& wk, FawPos& ps, uint32_t b, bool owned, Add& add) {
    if (wk.cr && b != '\n' && ps.advance()) {
        wk.flush(add);
        add.tile(ps.tile);
    }
    wk.template step<K>(b, owned, add);
    if (b != '\n' && !wk.hdr && !wk.cr && ps.advance()) {
        wk.flush(add);
        add.tile(ps.tile);
    }
}

// A lane's own bytes of the count: far_lane_count with the position.  At a header line start the pending addition is
// flushed and add.enter(ordinal, 0) names the next record's first tile.  Returns the header lines that start before the
// byte behind the lane's last.
template <int K, class Add>
__device__ inline uint32_t faw_lane_count(const uint32_t* w, uint32_t n, FaWalk& wk, FawPos& ps, uint32_t hb, Add& add) {
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
                    ps.template start<K>(0, ps.S);
                    add.enter(hb, ps.tile);
                    ++hb;
                }
                faw_step<K>(wk, ps, b, true, add);
            }
        }
    }
    return hb;
}

// What the count knows of a record (vk_faw_plan_kernel writes it).
struct FawRec {
    uint64_t ord0;     // joined bytes of the batch before the record's (the count subtracts the sample's first record's)
    uint64_t t_lo;     // the first tile the call needs
    uint32_t t_cnt;    // how many it needs from there on
    uint32_t slot0;    // the row of tile t_lo in the target buffer (d_hist, or the tile workspace)
};

#ifndef VK_FASTA_LANE_ONLY

// One workgroup.  recs has nrec + 1 entries (the last: ord0 alone).  m == 1: the rows are d_hist's, cap = nrows.  m > 1:
// they are the tile workspace's, cap of them; *tiles_used = how many are used.
__global__ __launch_bounds__(kFaThreads) void vk_faw_plan_kernel(const unsigned long long* rec_bases, const unsigned long long* win_first,
                                                                 uint64_t nrec, uint32_t N, uint32_t S, uint64_t row_lo, uint32_t nrows,
                                                                 uint32_t cap, FawRec* recs, uint32_t* tiles_used) {
    __shared__ unsigned long long s_wave[kFaThreads / 64];
    const uint32_t m = N / S;
    const uint64_t row_hi = row_lo > kFaNoWindow - nrows ? kFaNoWindow : row_lo + nrows;
    unsigned long long run_bases = 0, run_tiles = 0;
    for (uint64_t t = 0; t < nrec + 1; t += kFaThreads) {
        const uint64_t g = t + threadIdx.x;
        unsigned long long bases = 0, need = 0;
        uint64_t t_lo = 0, row0 = 0;
        if (g < nrec) {
            bases = rec_bases[g];
            const uint64_t first = win_first[g];
            const uint64_t nwin = first != kFaNoWindow && bases >= N ? (bases - N) / S + 1 : 0;
            if (nwin && first <= kFaNoWindow - nwin) {   // the record's rows [first, first + nwin), clipped to the range
                const uint64_t lo = first > row_lo ? first : row_lo;
                const uint64_t hi = first + nwin < row_hi ? first + nwin : row_hi;
                if (lo < hi) {
                    t_lo = lo - first;
                    row0 = lo - row_lo;
                    need = hi - lo + (m - 1u);   // (hi - lo <= nrows)
                }
            }
        }
        unsigned long long total_b, total_t;
        const unsigned long long before_b = fa_block_excl_sum(bases, s_wave, &total_b);
        const unsigned long long before_t = fa_block_excl_sum(need, s_wave, &total_t);
        if (g <= nrec) {
            const unsigned long long slot = m == 1 ? row0 : run_tiles + before_t;
            const unsigned long long room = slot < cap ? cap - slot : 0ull;
            recs[g] = FawRec{run_bases + before_b, t_lo, static_cast<uint32_t>(need < room ? need : room),
                             static_cast<uint32_t>(slot < cap ? slot : cap)};
        }
        run_bases += total_b;
        run_tiles += total_t;
    }
    if (threadIdx.x == 0) *tiles_used = static_cast<uint32_t>(run_tiles < cap ? run_tiles : cap);
}

// Where a lane's additions go: the workgroup's LDS table while it is in the (record, tile) that table belongs to, else the
// row of its tile, else nowhere.
template <int K>
struct FawAdd {
    static constexpr uint32_t NCODE = 1u << (2 * K);
    uint32_t* s_hist;          // the workgroup's LDS table (K <= 7)
    uint32_t* dest;            // the rows: cap of them
    const FawRec* recs;        // of the sample's records
    uint32_t nrec, cap;
    uint32_t own_ord;          // the record and tile the LDS table belongs to; kFaNoSlot: none
    uint64_t own_tile;
    uint64_t t_lo = 0;         // of the current record
    uint32_t t_cnt = 0, slot0 = 0;
    bool own_rec = false, to_lds = false;
    uint32_t* row = nullptr;

    __device__ inline void tile(uint64_t t) {
        to_lds = own_rec && t == own_tile;
        row = nullptr;
        if (to_lds || t < t_lo || t - t_lo >= t_cnt) return;
        const uint64_t sl = slot0 + (t - t_lo);
        if (sl < cap) row = dest + static_cast<size_t>(sl) * NCODE;
    }
    __device__ inline void enter(uint32_t ord, uint64_t t) {
        own_rec = ord == own_ord;
        t_cnt = 0;
        if (ord < nrec) {
            t_lo = recs[ord].t_lo;
            t_cnt = recs[ord].t_cnt;
            slot0 = recs[ord].slot0;
        }
        tile(t);
    }
    // can a tile of [a, b] have a row?
    __device__ inline bool needs(uint64_t a, uint64_t b) const { return t_cnt && b >= t_lo && a < t_lo + t_cnt; }
    __device__ inline void operator()(uint32_t code, uint32_t n) {
        if (to_lds) atomicAdd(s_hist + code, n);
        else if (row) atomicAdd(row + code, n);
    }
};

template <int K>
__global__ __launch_bounds__(kFaThreads) void vk_faw_count_kernel(const uint8_t* base, FaMeta m, const uint32_t* carry, const uint32_t* uhdr,
                                                                  const uint32_t* nrec_seen, FaRecs rc, const uint32_t* lane_idx,
                                                                  const unsigned long long* unit_ord, const FawRec* recs, uint32_t S,
                                                                  uint32_t* dest, uint32_t cap) {
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
    if (nrec == 0) return;
    const FawRec* srec = recs + g0;
    const uint64_t ord_base = srec[0].ord0;   // joined bytes of the batch before the sample's
    const uint32_t lanes = m.unit_bytes / kFaLaneBytes;
    // the records of this span: the one that enters it up to the last one that starts in it
    const uint32_t hb0 = uhdr[first + u0];
    const uint32_t hb1 = u1 < nunits ? uhdr[first + u1] : nrec_seen[s];
    const uint32_t own_ord = hb0 ? hb0 - 1u : 0u;
    uint32_t last = hb1 ? hb1 - 1u : 0u;
    if (last >= nrec) last = nrec - 1u;
    FawAdd<K> probe{s_hist, dest, srec, nrec, cap, kFaNoSlot, 0};
    // the entering record: its tiles from the one at the span's first byte to the one at the next span's first byte
    FawPos p0;
    int mine = 0;
    if (own_ord < nrec) {
        const uint64_t rec_ord = srec[own_ord].ord0 - ord_base;
        p0.template start<K>(unit_ord[first + u0] + (lane_idx[(first + u0) * lanes] & kFaIdxOrd) - rec_ord, S);
        const uint64_t t_end = u1 < nunits ? (unit_ord[first + u1] + (lane_idx[(first + u1) * lanes] & kFaIdxOrd) - rec_ord) / S : kFaNoWindow;
        probe.enter(own_ord, p0.tile);
        mine = t_end >= p0.tile && probe.needs(p0.tile, t_end) ? 1 : 0;
    }
    for (uint64_t r = static_cast<uint64_t>(own_ord) + 1u + threadIdx.x; r <= last; r += kFaThreads) mine |= srec[r].t_cnt ? 1 : 0;
    if (!__syncthreads_or(mine)) return;   // (uniform) none of their tiles is needed: the text is not read
    uint32_t* own_row = own_ord < nrec ? probe.row : nullptr;
    const bool lds_on = LDSH && own_row;
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
        FawAdd<K> add{s_hist, dest, srec, nrec, cap, lds_on ? own_ord : kFaNoSlot, p0.tile};
        FawPos ps;
        ps.S = S;
        if (hb) {
            const uint32_t cur = hb - 1u;
            const uint64_t q = unit_ord[first + u] + (lane_idx[(first + u) * lanes + threadIdx.x] & kFaIdxOrd);
            ps.template start<K>(cur < nrec ? q - (srec[cur].ord0 - ord_base) : 0ull, S);
            add.enter(cur, ps.tile);
        }
        // (lanes that left at n == 0 are the last ones of the workgroup: a wave that votes has its lane 0 here)
        const uint32_t hb_w = __shfl(hb, 0, 64);
        const unsigned long long tile_w = __shfl(static_cast<unsigned long long>(ps.tile), 0, 64);
        // (the k-mers a lane emits start at its own sequence bytes: K - 1 behind the position up to 63 further)
        constexpr int32_t REACH = static_cast<int32_t>(kFaLaneBytes) + K - 1;
        const bool plain = !__any(nh != 0 || n != kFaLaneBytes || hb == 0 || hb != hb_w || ps.tile != tile_w ||
                                  ps.r > static_cast<int32_t>(S) - REACH);
        if (plain) {
            // the whole wave lies in one tile of one record, holds no header line start and no seam, and no lane of it is
            // cut short by the sample's end
            if (!add.to_lds && !add.row) continue;
            FaAdd<K> one{add.to_lds ? s_hist : add.row};
#pragma unroll
            for (uint32_t i = 0; i < kFaLaneBytes; ++i) wk.template step<K>(fa_byte(w, i), true, one);
            for (uint64_t p = c0 + n; p < len && wk.template more<K>(); ++p) wk.template step<K>(text[p], false, one);
            wk.flush(one);
            continue;
        }
        // in a record none of whose tiles within reach of this lane is needed, and no other begins here
        if (nh == 0 && !add.to_lds && !add.needs(ps.tile, ps.tile + static_cast<uint32_t>(ps.r + REACH) / S)) continue;
        (void)faw_lane_count<K>(w, n, wk, ps, hb, add);
        for (uint64_t p = c0 + n; p < len && wk.template more<K>(); ++p) faw_step<K>(wk, ps, text[p], false, add);
        wk.flush(add);
    }
    if (lds_on) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < NCODE; i += kFaThreads) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(own_row + i, v);
        }
    }
}

// m > 1.  A workgroup per (tile row x of the workspace, chunk of codes): x is tile j of the record whose tiles hold it;
// if the m tiles from it on are the record's, they are a window, and its row of d_hist is their sum.
__global__ __launch_bounds__(kFaThreads) void vk_faw_sum_kernel(const FawRec* recs, const unsigned long long* win_first, uint64_t nrec,
                                                                const uint32_t* tiles_used, const uint32_t* tiles, uint32_t ncode, uint32_t m,
                                                                uint64_t row_lo, uint32_t nrows, uint32_t* hist) {
    const uint32_t chunks = ncode / kFawSumCodes;
    const uint32_t x = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (x >= *tiles_used) return;
    uint64_t lo = 0, hi = nrec;   // the last record whose first tile row is <= x: the one that holds it
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (recs[mid].slot0 <= x) lo = mid; else hi = mid;
    }
    const FawRec r = recs[lo];
    const uint32_t j = x - r.slot0;
    if (x < r.slot0 || j >= r.t_cnt || r.t_cnt - j < m) return;
    const uint64_t row = win_first[lo] + r.t_lo + j - row_lo;
    if (row >= nrows) return;
    const uint32_t* src = tiles + static_cast<size_t>(x) * ncode + chunk * kFawSumCodes;
    uint32_t* dst = hist + static_cast<size_t>(row) * ncode + chunk * kFawSumCodes;
    for (uint32_t c = threadIdx.x; c < kFawSumCodes; c += kFaThreads) {
        uint32_t sum = 0;
        for (uint32_t t = 0; t < m; ++t) sum += src[static_cast<size_t>(t) * ncode + c];
        dst[c] = sum;
    }
}

#endif  // VK_FASTA_LANE_ONLY

}  // namespace

#endif  // VK_FASTA_WINDOWS_H
