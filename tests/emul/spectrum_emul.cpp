// spectrum_emul.cpp -- CPU emulation of the lane-local device code of the k-mer spectrum (test only).
//
// Compiles the product's own csrc/vk_spectrum.h for the host (VK_SPECTRUM_LANE_ONLY and VK_SCREEN_LANE_ONLY: sp_taken,
// sp_insert, sp_count, sp_bin, and from vk_screen.h sc_code, sc_pack8, sc_window, sc_tile, sc_key, sc_mix) and runs a
// sample the way the kernels cut it, a lane at a time:
//   a read: tile after tile (sc_tile), the tile's bases packed eight at a time (sc_pack8) into code and mask words laid
//   out as vk_sp_count_kernel lays them out in LDS, then a lane per window position: sc_window, sc_key, sc_mix, sp_taken,
//   sp_count with one occurrence;
//   the histogram: sp_bin of every slot's count, as vk_sp_hist_kernel's lanes take them.
// The keys, the counts, every read and the code and mask words lie in heap blocks of exactly their size, so under the
// address sanitizer a probe past the table, a byte read past a read or a word read past the tile is an error.  A table
// without a free slot must end in VK_SPEC_TABLE_FULL and the program must end: the test runs it under a time limit.
//
// What it does NOT cover: the kernels themselves -- the record index and the framing, the race of concurrent
// compare-and-swaps and adds, the in-wave merge of equal keys, the wave's sums and their flush, the workgroups' cut of
// the slots: tests/test_gpu_spectrum.py.
//
// A stand-alone program:  spectrum_emul IN OUT TILE
//   IN:  samples, each u32 k, u32 every, u32 nslots, u32 reads, per read u32 length and its sequence line.
//   OUT: per sample u32 status (0 or VK_SPEC_TABLE_FULL), then u64 row[261].
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
#include "vk_spectrum.h"

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "spectrum_emul: %s\n", what);
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
    uint32_t K, every, tile;
    uint64_t nslots;
    std::unique_ptr<uint64_t[]> keys;
    std::unique_ptr<uint32_t[]> counts;
    uint64_t row[kSpNstat] = {};
    bool full = false;
};

// A read, tile by tile, as a wavefront of vk_sp_count_kernel takes it (without the merge: a lane per window adds 1).
void count_read(Sample& s, const uint8_t* seq, uint32_t L) {
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
            ++s.row[2];
            const uint64_t key = sc_key(fw, s.K), mix = sc_mix(key);
            if (!sp_taken(mix, s.every)) continue;
            ++s.row[3];
            if (!sp_count(s.keys.get(), s.counts.get(), s.nslots, key, mix, 1u)) s.full = true;
        }
        covered += nw;
        t0 += nw;
    }
    if (covered != (L >= s.K ? L - s.K + 1 : 0u)) die("the tiles do not cover the read's windows once each");
    ++s.row[0];
    s.row[1] += L;
}

void histogram(Sample& s) {
    for (uint64_t i = 0; i < s.nslots; ++i) {
        const uint32_t b = sp_bin(s.counts[i]);
        if ((b < kSpBins) != (s.keys[i] != kScEmpty)) die("a held slot without a count, or a count without a key");
        if (b < kSpBins) {
            ++s.row[kSpHistAt + b];
            ++s.row[4];
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) die("usage: spectrum_emul IN OUT TILE");
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
        s.tile = tile;
        if (s.K < kScMinK || s.K > kScMaxK || s.every < 1 || s.nslots < kScMinSlots || (s.nslots & (s.nslots - 1))) die("bad sample");
        s.keys.reset(new uint64_t[s.nslots]);
        s.counts.reset(new uint32_t[s.nslots]);
        for (uint64_t i = 0; i < s.nslots; ++i) {
            s.keys[i] = kScEmpty;
            s.counts[i] = 0;
        }
        const uint32_t nreads = get32(in, &at);
        for (uint32_t r = 0; r < nreads; ++r) {
            const uint32_t L = get32(in, &at);
            if (at + L > in.size()) die("bad read");
            std::unique_ptr<uint8_t[]> seq(new uint8_t[L ? L : 1]);   // a heap block of exactly the read
            memcpy(seq.get(), in.data() + at, L);
            at += L;
            count_read(s, seq.get(), L);
        }
        histogram(s);
        if (s.full) memset(s.row, 0, sizeof s.row);
        put(out, s.full ? kSpTableFull : 0u);
        for (uint64_t v : s.row) put(out, v);
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) die("cannot write OUT");
    fclose(f);
    return 0;
}
