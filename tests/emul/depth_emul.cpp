// depth_emul.cpp -- CPU emulation of the lane-local device code of the depth filter (test only).
//
// Compiles the product's own csrc/vk_depth.h for the host (VK_SPECTRUM_LANE_ONLY and VK_SCREEN_LANE_ONLY: sp_find, dp_bin,
// dp_kept, dp_decide, dp_lane_bin, dp_median_bin, and from vk_spectrum.h and vk_screen.h what the spectrum's emulation
// takes) and runs a sample the way the kernels cut it, a lane at a time:
//   the table: every read counted as tests/emul/spectrum_emul.cpp counts it (sp_count with one occurrence);
//   a read: tile after tile (sc_tile), the tile's bases packed eight at a time (sc_pack8) into code and mask words laid
//   out as vk_dp_match_kernel lays them out in LDS, then a lane per window position: sc_window, sc_key, sc_mix, sp_taken,
//   sp_find and one count, dp_bin into the read's 256 bins, the three sums; behind the last tile dp_median_bin (the
//   lanes' walk over four bins each, one lane after the other) and dp_decide; the bins cleared.
// The keys, the counts, every read and the code and mask words lie in heap blocks of exactly their size, so under the
// address sanitizer a probe past the table, a byte read past a read or a word read past the tile is an error.
//
//   depth_emul --probes: the two probes that only the emulation covers -- a key absent from a table with free slots has
//   no slot (depth 0), and a key absent from a 1,024-slot table WITHOUT a free slot has none either, after 1,024 probes:
//   the walk ends (the test runs the program under a time limit).
//
// What it does NOT cover: the kernels themselves -- the record index and the framing, the wave's ballots and sums and
// their flush, the LDS histogram's adds and the wave's scan over it, the copy of the kept records:
// tests/test_gpu_depth.py.
//
// A stand-alone program:  depth_emul IN OUT TILE
//   IN:  samples, each u32 k, u32 every, u32 nslots, u32 lo, u32 hi, u32 reads, per read u32 length and its sequence line.
//   OUT: per sample u32 status (0 or VK_SPEC_TABLE_FULL), u64 row[261], then a byte per read: kept or not.
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
inline void sp_add(uint32_t* p, uint32_t n) { *p += n; }
#define VK_SCREEN_LANE_ONLY
#define VK_SPECTRUM_LANE_ONLY
#include "vk_depth.h"

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "depth_emul: %s\n", what);
    exit(2);
}

uint32_t get32(const std::vector<uint8_t>& in, size_t* at) {
    if (*at + 4 > in.size()) die("short input");
    uint32_t v;
    memcpy(&v, in.data() + *at, 4);
    *at += 4;
    return v;
}

template <class T>
void put(std::vector<uint8_t>& out, T v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    out.insert(out.end(), p, p + sizeof(T));
}

struct Sample {
    uint32_t K, every, tile, lo, hi;
    uint64_t nslots;
    std::unique_ptr<uint64_t[]> keys;
    std::unique_ptr<uint32_t[]> counts;
    std::unique_ptr<uint32_t[]> hist;   // a wavefront's 256 bins
    uint64_t row[kDpNstat] = {};
    bool full = false;
};

// A read, tile by tile, as a wavefront takes it; per taken window f(key, mix).
template <class F>
void walk_read(const Sample& s, const uint8_t* seq, uint32_t L, F f) {
    const size_t ncode = s.tile / 16 + 2, nmask = s.tile / 32 + 1;   // (the kernel's arrays, at this tile size)
    std::unique_ptr<uint32_t[]> codes(new uint32_t[ncode]), masks(new uint32_t[nmask]);
    for (size_t i = 0; i < ncode; ++i) codes[i] = 0xA5A5A5A5u;   // (what a tile leaves behind is anything)
    for (size_t i = 0; i < nmask; ++i) masks[i] = 0x5A5A5A5Au;
    uint16_t* codes16 = reinterpret_cast<uint16_t*>(codes.get());
    uint8_t* masks8 = reinterpret_cast<uint8_t*>(masks.get());
    uint32_t t0 = 0, nb, nw, covered = 0;
    while (sc_tile(t0, L, s.tile, s.K, &nb, &nw)) {
        if (nb > s.tile || t0 + nb > L || nw != nb - s.K + 1) die("a tile past the read");
        for (uint32_t c = 0; c < (nb + 7u) / 8u; ++c) {
            uint16_t code;
            uint8_t mask;
            sc_pack8(seq + t0 + 8u * c, std::min(8u, nb - 8u * c), &code, &mask);
            if ((c ^ 1u) >= 2 * ncode || (c ^ 3u) >= 4 * nmask) die("a chunk past the words");
            codes16[c ^ 1u] = code;
            masks8[c ^ 3u] = mask;
        }
        for (uint32_t p = 0; p < nw; ++p) {
            uint64_t fw;
            if (!sc_window(codes.get(), masks.get(), p, s.K, &fw)) continue;
            const uint64_t key = sc_key(fw, s.K), mix = sc_mix(key);
            if (sp_taken(mix, s.every)) f(key, mix);
        }
        covered += nw;
        t0 += nw;
    }
    if (covered != (L >= s.K ? L - s.K + 1 : 0u)) die("the tiles do not cover the read's windows once each");
}

// A read against the table, as a wavefront of vk_dp_match_kernel decides it.
bool filter_read(Sample& s, const uint8_t* seq, uint32_t L) {
    uint32_t n = 0, below = 0, atmost = 0;
    walk_read(s, seq, L, [&](uint64_t key, uint64_t mix) {
        const uint64_t slot = sp_find(s.keys.get(), s.nslots, key, mix);
        if (slot != kSpNoSlot && slot >= s.nslots) die("a slot past the table");
        const uint32_t c = slot == kSpNoSlot ? 0u : s.counts[slot];
        ++n;
        below += c < s.lo ? 1u : 0u;
        atmost += c <= s.hi ? 1u : 0u;
        const uint32_t b = dp_bin(c);
        if (b >= kDpBins) die("a bin past the histogram");
        ++s.hist[b];
    });
    const uint32_t mbin = dp_median_bin(s.hist.get(), n);
    if (mbin >= kDpBins) die("a median past the histogram");
    uint32_t sum = 0;
    for (uint32_t i = 0; i < kDpBins; ++i) {
        sum += s.hist[i];
        s.hist[i] = 0;   // (clean for the next read)
    }
    if (sum != n) die("the bins do not sum to the read's taken windows");
    const bool kept = dp_decide(n, below, atmost, s.lo);
    ++s.row[0];
    s.row[2] += L;
    if (kept) {
        ++s.row[1];
        s.row[3] += L;
    }
    if (n == 0) ++s.row[4];
    ++s.row[kDpHistAt + mbin];
    return kept;
}

int probes() {
    const uint64_t nslots = kScMinSlots;
    std::unique_ptr<uint64_t[]> keys(new uint64_t[nslots]);
    const uint64_t absent = 0x123456789ull, mix = sc_mix(absent);
    // free slots all around: the walk ends at the first
    for (uint64_t i = 0; i < nslots; ++i) keys[i] = kScEmpty;
    for (uint64_t k = 1; k <= 600; ++k) {
        if (k == absent) die("the probe's key is among the held ones");
        if (sp_insert(keys.get(), nslots, k, sc_mix(k)) == kSpNoSlot) die("a table of 1,024 slots took no 600 keys");
    }
    if (sp_find(keys.get(), nslots, absent, mix) != kSpNoSlot) die("an absent key has a slot");
    for (uint64_t k = 1; k <= 600; ++k) {
        const uint64_t slot = sp_find(keys.get(), nslots, k, sc_mix(k));
        if (slot == kSpNoSlot || keys[slot] != k) die("a held key is not found");
    }
    // no free slot: the walk ends after nslots probes
    for (uint64_t i = 0; i < nslots; ++i) keys[i] = 1000000ull + i;
    for (uint64_t start = 0; start < nslots; start += 341)
        if (sp_find(keys.get(), nslots, absent, start) != kSpNoSlot) die("an absent key has a slot in a table without a free one");
    if (sp_find(keys.get(), nslots, 1000000ull + 5, 6) != 5) die("a held key behind the wrap-around is not found");
    printf("ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--probes")) return probes();
    if (argc != 4) die("usage: depth_emul IN OUT TILE | depth_emul --probes");
    const uint32_t tile = static_cast<uint32_t>(atoi(argv[3]));
    if (tile < 64 || tile % 64 || tile > kScMaxTile) die("bad tile");
    std::vector<uint8_t> in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) die("cannot read IN");
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + n);
        fclose(f);
    }
    std::vector<uint8_t> out;
    size_t at = 0;
    while (at < in.size()) {
        Sample s;
        s.K = get32(in, &at);
        s.every = get32(in, &at);
        s.nslots = get32(in, &at);
        s.lo = get32(in, &at);
        s.hi = get32(in, &at);
        s.tile = tile;
        if (s.K < kScMinK || s.K > kScMaxK || s.every < 1 || s.nslots < kScMinSlots || (s.nslots & (s.nslots - 1)) || s.lo > s.hi)
            die("bad sample");
        s.keys.reset(new uint64_t[s.nslots]);
        s.counts.reset(new uint32_t[s.nslots]);
        s.hist.reset(new uint32_t[kDpBins]());
        for (uint64_t i = 0; i < s.nslots; ++i) {
            s.keys[i] = kScEmpty;
            s.counts[i] = 0;
        }
        const uint32_t nreads = get32(in, &at);
        std::vector<std::unique_ptr<uint8_t[]>> reads;
        std::vector<uint32_t> lens;
        for (uint32_t r = 0; r < nreads; ++r) {
            const uint32_t L = get32(in, &at);
            if (at + L > in.size()) die("bad read");
            reads.emplace_back(new uint8_t[L ? L : 1]);   // a heap block of exactly the read
            memcpy(reads.back().get(), in.data() + at, L);
            lens.push_back(L);
            at += L;
        }
        for (uint32_t r = 0; r < nreads; ++r)
            walk_read(s, reads[r].get(), lens[r], [&](uint64_t key, uint64_t mix) {
                if (!sp_count(s.keys.get(), s.counts.get(), s.nslots, key, mix, 1u)) s.full = true;
            });
        std::vector<uint8_t> flags(nreads, 0);
        if (!s.full)
            for (uint32_t r = 0; r < nreads; ++r) flags[r] = filter_read(s, reads[r].get(), lens[r]) ? 1 : 0;
        put(out, s.full ? kSpTableFull : 0u);
        for (uint64_t v : s.row) put(out, v);
        out.insert(out.end(), flags.begin(), flags.end());
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) die("cannot write OUT");
    fclose(f);
    return 0;
}
