// fasta_emul.cpp -- CPU emulation of the lane-local device code of the FASTA count (test only).
//
// Compiles the product's own csrc/vk_fasta.h for the host (VK_FASTA_LANE_ONLY: FaWalk, fa_lane_key, fa_code, fa_byte) and
// runs a sample the way the kernels cut it: unit after unit, lane after lane, each lane with the 64 bytes it would have
// loaded, the state that enters it, its walk over its own bytes and its read forward past them.
//
// What it does NOT cover: the kernels themselves.  fa_load's bounds, the scans (fa_block_excl_max, vk_fa_scan_kernel;
// here a running maximum in lane order, which is what they compute), fa_locate, the atomics and the LDS histogram exist
// only on the GPU: tests/test_gpu_fasta.py runs them.
//
// A stand-alone program:  fasta_emul IN OUT K UNIT_BYTES
//   IN:  cases, each a u32 length and the bytes.   OUT: per case u32 status, u64 bases, u32 hist[4^K].
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define VK_FASTA_LANE_ONLY
#include "vk_fasta.h"

namespace {

struct HostAdd {
    uint32_t* hist;
    void operator()(uint32_t code, uint32_t n) { hist[code] += n; }
};

template <int K>
void count(const uint8_t* text, uint64_t len, uint32_t unit, uint32_t* hist, uint64_t* bases, uint32_t* status) {
    *status = len && text[0] != '>' ? 1u : 0u;
    *bases = 0;
    if (*status) return;
    HostAdd add{hist};
    uint32_t carry = 0;   // the state that enters the unit: vk_fa_scan_kernel's
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
            FaWalk wk;
            wk.hdr = excl ? excl & 1u : carry;
            wk.ls = first_ls ? 1u : 0u;
            for (uint32_t i = 0; i < n; ++i) wk.step<K>(fa_byte(w, i), true, add);
            for (uint64_t p = c0 + n; p < len && wk.more<K>(); ++p) wk.step<K>(text[p], false, add);
            wk.flush(add);
            *bases += wk.bases;
            if (lk) excl = ((lane + 1u) << 1) | (lk & 1u);
        }
        if (excl) carry = excl & 1u;
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: fasta_emul IN OUT K UNIT_BYTES\n");
        return 2;
    }
    const int k = atoi(argv[3]);
    const uint32_t unit = static_cast<uint32_t>(strtoul(argv[4], nullptr, 10));
    if (k < 5 || k > 9 || unit < kFaLaneBytes || unit % kFaLaneBytes || unit > kFaUnitBytes) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<uint32_t> hist(static_cast<size_t>(1) << (2 * k));
    uint32_t len;
    while (fread(&len, 4, 1, in) == 1) {
        std::vector<uint8_t> text(len);   // exactly len bytes: a read past the sample is the sanitizer's to find
        if (len && fread(text.data(), 1, len, in) != len) return 3;
        std::fill(hist.begin(), hist.end(), 0u);
        uint64_t bases = 0;
        uint32_t status = 0;
        switch (k) {
            case 5: count<5>(text.data(), len, unit, hist.data(), &bases, &status); break;
            case 6: count<6>(text.data(), len, unit, hist.data(), &bases, &status); break;
            case 7: count<7>(text.data(), len, unit, hist.data(), &bases, &status); break;
            case 8: count<8>(text.data(), len, unit, hist.data(), &bases, &status); break;
            default: count<9>(text.data(), len, unit, hist.data(), &bases, &status); break;
        }
        fwrite(&status, 4, 1, out);
        fwrite(&bases, 8, 1, out);
        fwrite(hist.data(), 4, hist.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
