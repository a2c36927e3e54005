// vk_fasta_spectrum.h -- `image / query --from-fasta --genome-spectrum`: the k-mer spectrum of assemblies, counted straight
// from FASTA text in HBM into vk_spectrum.h's counting tables.  Part of the one translation unit vkimg.hip (device code for
// gfx950; see the notes there).
//
// The rule ("`--genome-spectrum`: the rule"; tests/fasta_spectrum_ref.py is the same rule in Python, twice):
// lines, header lines and records are vk_fasta.h's; bases, windows and keys are the screen's (vk_screen.h: ACGT of either
// case, every window of K = 16..31 unbroken bases gives sc_key; a window runs across line ends, never across a header line
// or any other byte); a key is TAKEN as in vk_spectrum.h, (sc_mix(key) >> 32) % every == 0, and every occurrence of a taken
// key counts.  A sample's row is vk_spectrum.h's with records (header lines) where reads stand and vk_fasta.h's bases
// (joined sequence bytes of every class): records, bases, windows, taken windows, distinct, hist[256].
//
// Work is cut by BYTES as in vk_fa_count_kernel: a lane owns kFaLaneBytes of text, a workgroup a span of units of one
// sample.  A lane's own bytes come in with fa_load's four 16-byte loads and are walked from registers; only the up to K - 1
// further bases its open windows need behind its last byte are read from memory, a byte at a time.  The lane owns the
// windows that START in its bytes.  It rolls the 2K-bit window and its reverse complement (ScWalk::step's rule, written
// with selects as FaWalk is; a word of the lane's registers at a time, four steps unrolled), folds a run of equal consecutive
// keys (a homopolymer) into one addition, asks sp_taken before any table access, and places the key with sp_insert and the
// no-return add sp_add.  Lanes of one wave instruction hold text 64 bytes apart: their keys are unrelated, nothing is
// merged across lanes.
//
// Launch sequence of vk_spectrum_fasta_device:
//   vk_fa_summary_kernel / vk_fa_scan_kernel   the header state that enters every unit; the status words (vk_fasta.h, unchanged)
//   vk_sp_init_kernel                          keys all ones, counts zero (vk_spectrum.h, unchanged)
//   vk_fs_count_kernel                         the count; records, bases, windows, taken windows summed per wave, one atomic
//                                              per wave and total; a key without a slot raises VK_SPEC_TABLE_FULL, the
//                                              sample's other workgroups stop at their next unit
//   vk_sp_hist_kernel / vk_sp_finish_kernel    distinct and the histogram; a sample with a status gets an all-zero row
//                                              (vk_spectrum.h, unchanged)
//
// The lane-local code (FsWalk, FsTable) compiles for the host: tests/emul/fasta_spectrum_emul.cpp runs it, a lane at a time,
// against tests/fasta_spectrum_ref.py.
#ifndef VK_FASTA_SPECTRUM_H
#define VK_FASTA_SPECTRUM_H

#include <cstdint>

#include "vk_fasta.h"
#include "vk_spectrum.h"

namespace {

// A lane's walk over the text, a byte at a time, from its first byte on: FaWalk with ScWalk's 2K-bit window and its reverse
// complement rolled along.  `owned` bytes are the lane's own (they count towards `bases` and `records`); behind them the
// walk goes on with owned = false for as long as more() says.
struct FsWalk {
    uint64_t fw = 0, rc = 0;
    uint64_t pend_key = 0;   // additions of one key not yet made
    uint32_t pend_n = 0;
    uint32_t run = 0;        // bases since the walk began or the last break
    uint32_t hdr = 0;        // inside a header line
    uint32_t ls = 0;         // the next byte starts a line
    uint32_t cr = 0;         // a '\r' of a sequence line waits for the byte behind it
    uint32_t cr_owned = 0;
    uint32_t extra = 0;      // bases taken behind the lane's own bytes
    uint32_t bases = 0;      // sequence bytes (joined bytes, every class) among the lane's own
    uint32_t records = 0;    // header lines that start among the lane's own bytes
    uint32_t windows = 0;    // windows that start among the lane's own bytes

    // add(key, n): n occurrences of key, a run of consecutive windows
    template <class Add>
    __device__ inline void step(uint32_t b, bool owned, uint32_t K, Add& add) {
        const bool nl = b == '\n';
        // '\r' + '\n' is a line end; before anything else the '\r' is a byte like any other non-base
        const bool cr_break = cr && !nl;
        bases += cr_break ? cr_owned : 0u;
        run = cr_break ? 0u : run;
        const bool header = ls && b == '>';
        records += header && owned ? 1u : 0u;
        hdr = ls ? (header ? 1u : 0u) : hdr;
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
        const uint64_t mask = (1ull << (2u * K)) - 1u;
        fw = base ? ((fw << 2) | c) & mask : fw;
        rc = base ? (rc >> 2) | (static_cast<uint64_t>(3u - c) << (2u * K - 2u)) : rc;
        extra += base && !owned ? 1u : 0u;
        // a window that started among the lane's own bytes (extra <= K - 1)
        const bool emit = base && run >= K;
        const uint64_t key = fw < rc ? fw : rc;
        const bool same = pend_n && pend_key == key;
        if (emit && !same && pend_n) add(pend_key, pend_n);
        windows += emit ? 1u : 0u;
        pend_n = emit ? (same ? pend_n + 1u : 1u) : pend_n;
        pend_key = emit ? key : pend_key;
    }

    // behind the lane's own bytes: windows are still open, or a '\r' still waits for its verdict
    __device__ inline bool more(uint32_t K) const { return (run > 0 || cr) && extra < K - 1u; }

    template <class Add>
    __device__ inline void flush(Add& add) {
        if (pend_n) add(pend_key, pend_n);
        pend_n = 0;
    }
};

// Where a lane's additions go: the sample's table.  sp_taken before any table access; after a key found no slot the lane
// touches the table no more.
struct FsTable {
    uint64_t* keys;
    uint32_t* counts;
    uint64_t nslots;
    uint32_t every;
    uint32_t taken = 0;   // taken windows
    uint32_t full = 0;

    __device__ inline void operator()(uint64_t key, uint32_t n) {
        const uint64_t mix = sc_mix(key);
        if (!sp_taken(mix, every)) return;
        taken += n;
        if (full) return;
        if (!sp_count(keys, counts, nslots, key, mix, n)) full = 1u;
    }
};

#ifndef VK_FASTA_SPECTRUM_LANE_ONLY

__global__ __launch_bounds__(kFaThreads) void vk_fs_count_kernel(const uint8_t* base, FaMeta m, const uint32_t* carry, SpParams P,
                                                                 uint32_t* status, unsigned long long* rows) {
    __shared__ uint32_t s_wave[kFaThreads / 64];
    uint64_t u0, u1;
    const uint32_t s = fa_locate(m, blockIdx.x, &u0, &u1);
    const uint8_t* text = base + m.offs[s];
    const uint64_t len = m.lens[s];
    if (text[0] != '>') return;   // VK_ST_BAD_START (a sample with a workgroup is not empty): its row is zeroed at the end
    FsTable add{P.keys + P.slot_base[s], P.counts + P.slot_base[s], P.nslots[s], P.every};
    const uint32_t K = P.K;
    uint32_t n_rec = 0, n_bases = 0, n_win = 0;
    for (uint64_t u = u0; u < u1; ++u) {
        // a table that some lane found full: the walk is skipped, the loop and its barriers go on (waves may read different
        // values here, so the test guards nothing that meets a barrier)
        const bool stop = __hip_atomic_load(status + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        uint32_t w[kFaLaneBytes / 4], n;
        uint64_t c0;
        fa_load(text, len, u, m.unit_bytes, w, &c0, &n);
        const bool first_ls = n && (c0 == 0 || text[c0 - 1] == '\n');
        const uint32_t lk = fa_lane_key(w, n, first_ls);
        uint32_t total;
        const uint32_t excl = fa_block_excl_max(lk ? ((threadIdx.x + 1u) << 1) | (lk & 1u) : 0u, s_wave, &total);
        if (n == 0 || stop) continue;   // (uniform calls above; nothing below meets a barrier)
        FsWalk wk;
        wk.hdr = excl ? excl & 1u : carry[m.unit_first[s] + u];
        wk.ls = first_ls ? 1u : 0u;
        // a word at a time, four steps unrolled: the table access is inlined into every step, and sixty-four copies of it
        // spill scalar registers inside its probe loop (the word's index is the wave's: a relative register move, no scratch)
#pragma unroll 1
        for (uint32_t q = 0; q < kFaLaneBytes / 4; ++q) {
            const uint32_t word = w[q];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (4u * q + j < n) wk.step((word >> (8u * j)) & 255u, true, K, add);
        }
        for (uint64_t p = c0 + n; p < len && wk.more(K); ++p) wk.step(text[p], false, K, add);
        wk.flush(add);
        n_rec += wk.records;
        n_bases += wk.bases;
        n_win += wk.windows;
    }
    // the sample's totals: a sum per wave (a lane's span holds at most kFaSpanUnits * kFaLaneBytes bytes: the sums fit 32
    // bits), one atomic each
    uint32_t n_taken = add.taken, full = add.full;
    for (uint32_t d = 32; d; d >>= 1) {
        n_rec += __shfl_down(n_rec, d, 64);
        n_bases += __shfl_down(n_bases, d, 64);
        n_win += __shfl_down(n_win, d, 64);
        n_taken += __shfl_down(n_taken, d, 64);
        full |= __shfl_down(full, d, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long* row = rows + static_cast<uint64_t>(kSpNstat) * s;
        if (n_rec) atomicAdd(row + 0, static_cast<unsigned long long>(n_rec));
        if (n_bases) atomicAdd(row + 1, static_cast<unsigned long long>(n_bases));
        if (n_win) atomicAdd(row + 2, static_cast<unsigned long long>(n_win));
        if (n_taken) atomicAdd(row + 3, static_cast<unsigned long long>(n_taken));
        if (full) atomicOr(status + s, kSpTableFull);   // (the sample's row is zeroed at the end)
    }
}

#endif  // VK_FASTA_SPECTRUM_LANE_ONLY

}  // namespace

#endif  // VK_FASTA_SPECTRUM_H
