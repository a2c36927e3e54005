// fasta_spectrum_emul.cpp -- CPU emulation of the lane-local device code of the assemblies' k-mer spectrum (test only).
//
// Compiles the product's own csrc/vk_fasta_spectrum.h for the host (VK_FASTA_SPECTRUM_LANE_ONLY: FsWalk, FsTable, with
// vk_fasta.h's fa_lane_key / fa_byte and vk_spectrum.h's sp_taken / sp_insert / sp_count) and runs a sample the way
// vk_fs_count_kernel cuts it: unit after unit, lane after lane, each lane with the 64 bytes it would have loaded, the
// header state that enters it, its walk over its own bytes from those registers and its read forward past them, every
// addition through FsTable into a table of the caller's size.
// The text lies in a heap block of exactly its size and the table in blocks of exactly nslots, so under the address
// sanitizer a byte read past the sample or a probe past the table is an error.
//
// What it does NOT cover: the kernels themselves.  fa_load's bounds, the scans (here a running maximum in lane order, which
// is what they compute), fa_locate, the race of concurrent compare-and-swaps, the wave sums, the early stop of a full
// table's other lanes, the histogram and finish kernels exist only on the GPU: tests/test_gpu_fasta_spectrum.py runs them.
//
// A library (tests/fasta_spectrum_emul_lib.py) and, with -DFASTA_SPECTRUM_EMUL_MAIN, a stand-alone program:
//   fasta_spectrum_emul IN OUT UNIT
//   IN:  samples, each u32 k, u32 every, u32 nslots, u32 length and the text.
//   OUT: per sample u32 status, u64 records, bases, windows, taken windows, additions, held; then held (u64 key, u32 count)
//        pairs in slot order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define __device__
#define __host__
// what the headers take from HIP: the 64-bit compare-and-swap of the insertion and the 32-bit add of the count
inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long cmp, unsigned long long val) {
    const unsigned long long old = *p;
    if (old == cmp) *p = val;
    return old;
}
static uint64_t g_adds = 0;   // additions that reached the table
inline void sp_add(uint32_t* p, uint32_t n) {
    *p += n;
    ++g_adds;
}
#define VK_FASTA_LANE_ONLY
#define VK_SCREEN_LANE_ONLY
#define VK_SPECTRUM_LANE_ONLY
#define VK_FASTA_SPECTRUM_LANE_ONLY
#include "vk_fasta_spectrum.h"

namespace {

// totals: records, bases, windows, taken windows, additions
void count(const uint8_t* text, uint64_t len, uint32_t K, uint32_t every, uint32_t unit, uint64_t nslots, uint64_t* keys,
           uint32_t* counts, uint64_t* totals, uint32_t* status) {
    for (uint64_t i = 0; i < nslots; ++i) {
        keys[i] = kScEmpty;
        counts[i] = 0;
    }
    for (int i = 0; i < 5; ++i) totals[i] = 0;
    *status = len && text[0] != '>' ? 1u : 0u;
    if (*status) return;
    g_adds = 0;
    uint32_t carry = 0;   // the state that enters the unit: vk_fa_scan_kernel's
    uint32_t full = 0;
    for (uint64_t ub = 0; ub < len; ub += unit) {
        uint32_t excl = 0;   // running maximum of the lanes' keys before this lane: fa_block_excl_max's
        for (uint32_t lane = 0; lane * kFaLaneBytes < unit; ++lane) {
            const uint64_t c0 = ub + static_cast<uint64_t>(lane) * kFaLaneBytes;
            if (c0 >= len) break;
            const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
            uint32_t w[kFaLaneBytes / 4];
            memset(w, 0xA5, sizeof w);   // (bytes past n are whatever the 16-byte loads bring)
            memcpy(w, text + c0, n);
            const bool first_ls = c0 == 0 || text[c0 - 1] == '\n';
            const uint32_t lk = fa_lane_key(w, n, first_ls);
            FsTable add{keys, counts, nslots, every};
            FsWalk wk;
            wk.hdr = excl ? excl & 1u : carry;
            wk.ls = first_ls ? 1u : 0u;
            for (uint32_t i = 0; i < n; ++i) wk.step(fa_byte(w, i), true, K, add);
            for (uint64_t p = c0 + n; p < len && wk.more(K); ++p) wk.step(text[p], false, K, add);
            wk.flush(add);
            totals[0] += wk.records;
            totals[1] += wk.bases;
            totals[2] += wk.windows;
            totals[3] += add.taken;
            full |= add.full;
            if (lk) excl = ((lane + 1u) << 1) | (lk & 1u);
        }
        if (excl) carry = excl & 1u;
    }
    totals[4] = g_adds;
    if (full) *status |= kSpTableFull;
}

}  // namespace

extern "C" int emul_fasta_spectrum(const uint8_t* text, uint64_t len, uint32_t K, uint32_t every, uint32_t unit, uint64_t nslots,
                                   uint64_t* keys, uint32_t* counts, uint64_t* totals, uint32_t* status) {
    if (K < kScMinK || K > kScMaxK || every < 1 || unit < kFaLaneBytes || unit % kFaLaneBytes || unit > kFaUnitBytes ||
        nslots < kScMinSlots || (nslots & (nslots - 1)))
        return 2;
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);   // a heap block of exactly len bytes
    if (len) memcpy(exact.get(), text, len);
    count(exact.get(), len, K, every, unit, nslots, keys, counts, totals, status);
    return 0;
}

#ifdef FASTA_SPECTRUM_EMUL_MAIN
int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: fasta_spectrum_emul IN OUT UNIT\n");
        return 2;
    }
    const uint32_t unit = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[4];
    while (fread(head, 4, 4, in) == 4) {
        const uint32_t K = head[0], every = head[1], nslots = head[2], len = head[3];
        std::vector<uint8_t> text(len);
        if (len && fread(text.data(), 1, len, in) != len) return 3;
        std::unique_ptr<uint64_t[]> keys(new uint64_t[nslots ? nslots : 1]);
        std::unique_ptr<uint32_t[]> counts(new uint32_t[nslots ? nslots : 1]);
        uint64_t totals[5];
        uint32_t status;
        if (emul_fasta_spectrum(text.data(), len, K, every, unit, nslots, keys.get(), counts.get(), totals, &status)) return 2;
        uint64_t held = 0;
        for (uint64_t i = 0; i < nslots; ++i) held += keys[i] != kScEmpty;
        fwrite(&status, 4, 1, out);
        fwrite(totals, 8, 5, out);
        fwrite(&held, 8, 1, out);
        for (uint64_t i = 0; i < nslots; ++i)
            if (keys[i] != kScEmpty) {
                fwrite(&keys[i], 8, 1, out);
                fwrite(&counts[i], 4, 1, out);
            }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
#endif
