// fasta_ladder_emul.cpp -- CPU emulation of the lane-local device code of the FASTA subsample ladder (test only).
//
// Compiles the product's own csrc/vk_fasta_ladder.h for the host (VK_FASTA_LANE_ONLY: fa_lane_bases, FaFragWalk with its
// ordinal bookkeeping, fragment tracking, skip test and emit condition, on top of vk_fasta.h's fa_lane_key, fa_code,
// fa_byte and vk_lane.h's sample_hash) and runs a sample the way the kernels cut it: first the index -- unit after unit,
// lane after lane, each lane's sequence bytes from the 64 bytes it would have loaded and the state that enters it, summed
// in lane order --, then every step: each lane starts from its index word, asks whether any of its fragments is taken,
// and only then walks its own bytes and reads forward past them.
//
// What it does NOT cover: the kernels themselves.  The loads and their bounds (fa_load, fa_load_lane), the scans
// (fa_block_excl_max, fa_block_excl_sum, vk_fa_scan_kernel, vk_fa_ordscan_kernel; here running values in lane order,
// which is what they compute), the pair and unit lookup, the atomics and the LDS histogram exist only on the GPU:
// tests/test_gpu_fasta_ladder.py runs them.
//
// A stand-alone program:  fasta_ladder_emul IN OUT K UNIT_BYTES
//   IN:  cases, each a u32 length, the bytes, a u32 number of steps and per step u32 L, u64 seed, u64 threshold, u64 shift.
//   OUT: per case u32 status, u64 bases and per step u64 taken, u32 n, then the n bins of the histogram that are not zero
//        as (u32 code, u32 count), in the order of the codes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define VK_FASTA_LANE_ONLY
#include "vk_fasta_ladder.h"

namespace {

struct HostAdd {
    uint32_t* hist;
    void operator()(uint32_t code, uint32_t n) { hist[code] += n; }
};

struct Index {
    std::vector<uint32_t> lane;       // per lane of every unit: vk_fa_ord_kernel's word
    std::vector<uint64_t> unit_ord;   // per unit: the ordinal of its first byte (vk_fa_ordscan_kernel's)
    uint64_t bases = 0;
};

void lane_bytes(const uint8_t* text, uint64_t c0, uint32_t n, uint32_t* w) {
    memset(w, 0xA5, kFaLaneBytes);   // (bytes past n are whatever the 16-byte loads bring)
    memcpy(w, text + c0, n);
}

Index build_index(const uint8_t* text, uint64_t len, uint32_t unit) {
    Index ix;
    const uint32_t lanes = unit / kFaLaneBytes;
    uint32_t carry = 0;
    for (uint64_t ub = 0; ub < len; ub += unit) {
        uint32_t excl = 0, before = 0;
        ix.unit_ord.push_back(ix.bases);
        for (uint32_t lane = 0; lane < lanes; ++lane) {
            const uint64_t c0 = ub + static_cast<uint64_t>(lane) * kFaLaneBytes;
            if (c0 >= len) {
                ix.lane.push_back(before);
                continue;
            }
            const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
            uint32_t w[kFaLaneBytes / 4];
            lane_bytes(text, c0, n, w);
            const bool first_ls = c0 == 0 || text[c0 - 1] == '\n';
            const uint32_t lk = fa_lane_key(w, n, first_ls);
            const uint32_t hdr = excl ? excl & 1u : carry;
            const uint32_t next = c0 + n < len ? text[c0 + n] : '\n';
            ix.lane.push_back(before | (hdr ? kFaIdxHdr : 0u) | (first_ls ? kFaIdxLs : 0u));
            before += fa_lane_bases(w, n, hdr, first_ls, next);
            if (lk) excl = ((lane + 1u) << 1) | (lk & 1u);
        }
        if (excl) carry = excl & 1u;
        ix.bases += before;
    }
    return ix;
}

template <int K>
void count(const uint8_t* text, uint64_t len, uint32_t unit, const Index& ix, const FaFrag& st, uint32_t* hist, uint64_t* taken) {
    HostAdd add{hist};
    const uint32_t lanes = unit / kFaLaneBytes;
    *taken = 0;
    for (uint64_t u = 0; u * unit < len; ++u) {
        for (uint32_t lane = 0; lane < lanes; ++lane) {
            const uint64_t c0 = u * unit + static_cast<uint64_t>(lane) * kFaLaneBytes;
            if (c0 >= len) break;
            const uint32_t n = len - c0 < kFaLaneBytes ? static_cast<uint32_t>(len - c0) : kFaLaneBytes;
            const uint32_t word = ix.lane[u * lanes + lane];
            FaFragWalk wk;
            wk.start(st, ix.unit_ord[u] + (word & kFaIdxOrd));
            if (!wk.any_taken(st, n)) continue;
            wk.hdr = word & kFaIdxHdr ? 1u : 0u;
            wk.ls = word & kFaIdxLs ? 1u : 0u;
            uint32_t w[kFaLaneBytes / 4];
            lane_bytes(text, c0, n, w);
            for (uint32_t i = 0; i < n; ++i) wk.step<K>(fa_byte(w, i), true, st, add);
            for (uint64_t p = c0 + n; p < len && wk.more<K>(); ++p) wk.step<K>(text[p], false, st, add);
            wk.flush(add);
            *taken += wk.taken;
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: fasta_ladder_emul IN OUT K UNIT_BYTES\n");
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
        const uint32_t status = len && text[0] != '>' ? 1u : 0u;
        const Index ix = build_index(text.data(), len, unit);
        const uint64_t bases = status ? 0 : ix.bases;
        fwrite(&status, 4, 1, out);
        fwrite(&bases, 8, 1, out);
        uint32_t nsteps;
        if (fread(&nsteps, 4, 1, in) != 1) return 3;
        for (uint32_t j = 0; j < nsteps; ++j) {
            FaFrag st;
            if (fread(&st.len, 4, 1, in) != 1 || fread(&st.seed, 8, 1, in) != 1 || fread(&st.threshold, 8, 1, in) != 1 ||
                fread(&st.shift, 8, 1, in) != 1)
                return 3;
            if (st.len < static_cast<uint32_t>(k)) return 2;
            std::fill(hist.begin(), hist.end(), 0u);
            uint64_t taken = 0;
            if (!status) {
                switch (k) {
                    case 5: count<5>(text.data(), len, unit, ix, st, hist.data(), &taken); break;
                    case 6: count<6>(text.data(), len, unit, ix, st, hist.data(), &taken); break;
                    case 7: count<7>(text.data(), len, unit, ix, st, hist.data(), &taken); break;
                    case 8: count<8>(text.data(), len, unit, ix, st, hist.data(), &taken); break;
                    default: count<9>(text.data(), len, unit, ix, st, hist.data(), &taken); break;
                }
            }
            fwrite(&taken, 8, 1, out);
            std::vector<uint32_t> bins;
            for (uint32_t c = 0; c < hist.size(); ++c) {
                if (hist[c]) {
                    bins.push_back(c);
                    bins.push_back(hist[c]);
                }
            }
            const uint32_t nbins = static_cast<uint32_t>(bins.size() / 2);
            fwrite(&nbins, 4, 1, out);
            if (nbins) fwrite(bins.data(), 4, bins.size(), out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
