// screen_emul.cpp -- CPU emulation of the lane-local device code of the read screen (test only).
//
// Compiles the product's own csrc/vk_screen.h for the host (VK_SCREEN_LANE_ONLY: sc_code, sc_revcomp, sc_key, sc_probe,
// sc_insert, sc_pack8, sc_window, sc_tile, ScWalk) and runs a case the way the kernels cut it.
//   The set: the reference is cut into units of UNIT bytes and lanes of 64; every lane's header state is what the scan
//   would hand it (computed here by a plain walk from the text's start), and the lane walks its own bytes and then reads
//   on while ScWalk::more says so -- exactly vk_sc_build_kernel's loop -- inserting every key with sc_insert.
//   A read: tile after tile (sc_tile), the tile's bases packed eight at a time (sc_pack8) into code and mask words laid
//   out as the kernel lays them out in LDS (u16 c ^ 1, byte c ^ 3), then a lane per window position: sc_window, sc_key,
//   sc_probe.  sc_window's result is also held against a plain restatement at every position, so every bit offset of a
//   window in its words is covered; sc_revcomp against a base-by-base one.
// The reference, the table, every read and the code and mask words lie in heap blocks of exactly their size (the words:
// what the kernel's LDS arrays hold for the tile size in use), so under the address sanitizer a byte read past the text, a
// probe past the table or a word read past the tile is an error.
//
// What it does NOT cover: the kernels themselves -- the header-state scan, the race of concurrent compare-and-swaps, the
// wave-wide sum of the hits and its early stop, the record index, the scan of the kept bytes, the write and pad
// kernels, the statistics: tests/test_gpu_screen.py.
//
// A stand-alone program:  screen_emul IN OUT TILE UNIT
//   IN:  cases, each u32 k, u32 nslots (0: the rule's), u32 fasta length, the fasta, u32 reads, per read u32 length and its
//        sequence line.
//   OUT: per case u32 status, u64 windows, u64 distinct, u64 nslots, the distinct keys sorted (u64 each), then per read
//        u32 hits.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define __device__
#define __host__
// what vk_screen.h takes from HIP: the 64-bit compare-and-swap of the insertion
inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long cmp, unsigned long long val) {
    const unsigned long long old = *p;
    if (old == cmp) *p = val;
    return old;
}
#define VK_SCREEN_LANE_ONLY
#include "vk_screen.h"

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "screen_emul: %s\n", what);
    exit(2);
}

template <class T>
std::unique_ptr<T[]> exact(const T* p, size_t n) {   // a heap block of exactly n elements
    std::unique_ptr<T[]> q(new T[n ? n : 1]);
    for (size_t i = 0; i < n; ++i) q[i] = p[i];
    return q;
}

struct SetResult {
    uint32_t status = 0;
    uint64_t windows = 0, distinct = 0, nslots = 0;
    std::unique_ptr<uint64_t[]> table;
};

// The header state at byte `at`, as the scan would state it: is the line that holds the byte a header line.
bool header_at(const uint8_t* text, uint64_t at) {
    uint64_t ls = at;
    while (ls > 0 && text[ls - 1] != '\n') --ls;
    return text[ls] == '>';
}

// One pass of the build over the text (insert = false: the count alone).
void build_pass(const uint8_t* text, uint64_t len, uint32_t K, uint32_t unit, bool insert, SetResult* res) {
    res->windows = 0;
    res->distinct = 0;
    if (len == 0 || text[0] != '>') return;
    for (uint64_t u0 = 0; u0 < len; u0 += unit)
        for (uint64_t c0 = u0; c0 < std::min<uint64_t>(u0 + unit, len); c0 += 64) {
            const uint64_t own_end = std::min<uint64_t>(std::min<uint64_t>(c0 + 64, u0 + unit), len);
            ScWalk wk;
            wk.ls = (c0 == 0 || text[c0 - 1] == '\n') ? 1u : 0u;
            wk.hdr = wk.ls ? 0u : (header_at(text, c0) ? 1u : 0u);
            uint64_t p = c0;
            while (p < len && (p < own_end || wk.more(K))) {
                uint64_t key;
                if (wk.step(text[p], p < own_end, K, &key)) {
                    ++res->windows;
                    if (insert) {
                        const uint32_t r = sc_insert(res->table.get(), res->nslots, key);
                        if (r == 2u) die("the table is full");
                        res->distinct += r;
                    }
                }
                ++p;
            }
        }
}

uint64_t plain_revcomp(uint64_t fw, uint32_t K) {   // base by base
    uint64_t rc = 0;
    for (uint32_t i = 0; i < K; ++i) {
        rc = (rc << 2) | (3u - (fw & 3u));
        fw >>= 2;
    }
    return rc;
}

// A read's hits, tile by tile, as a wavefront of vk_sc_match_kernel takes it (without the early stop).
uint32_t read_hits(const uint8_t* seq, uint32_t L, const SetResult& set, uint32_t K, uint32_t tile) {
    const size_t ncode = tile / 16 + 2, nmask = tile / 32 + 1;   // (the kernel's arrays, at this tile size)
    std::unique_ptr<uint32_t[]> codes(new uint32_t[ncode]), masks(new uint32_t[nmask]);
    for (size_t i = 0; i < ncode; ++i) codes[i] = 0xA5A5A5A5u;   // (what a tile leaves behind is anything)
    for (size_t i = 0; i < nmask; ++i) masks[i] = 0x5A5A5A5Au;
    uint16_t* codes16 = reinterpret_cast<uint16_t*>(codes.get());
    uint8_t* masks8 = reinterpret_cast<uint8_t*>(masks.get());
    uint32_t hits = 0, t0 = 0, nb, nw, covered = 0;
    while (sc_tile(t0, L, tile, K, &nb, &nw)) {
        if (nb > tile || t0 + nb > L || nw != nb - K + 1) die("a tile past the read");
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
            const bool ok = sc_window(codes.get(), masks.get(), p, K, &fw);
            // a plain restatement, from the bytes
            bool want_ok = true;
            uint64_t want = 0;
            for (uint32_t i = 0; i < K; ++i) {
                const uint32_t c = sc_code(seq[t0 + p + i]);
                if (c > 3u) want_ok = false;
                want = (want << 2) | (c & 3u);
            }
            if (ok != want_ok || (ok && fw != want)) die("sc_window differs from the bytes");
            if (ok) {
                if (sc_revcomp(fw, K) != plain_revcomp(fw, K)) die("sc_revcomp differs");
                if (sc_probe(set.table.get(), set.nslots, sc_key(fw, K))) ++hits;
            }
        }
        covered += nw;
        t0 += nw;
    }
    if (covered != (L >= K ? L - K + 1 : 0u)) die("the tiles do not cover the read's windows once each");
    return hits;
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

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) die("usage: screen_emul IN OUT TILE UNIT");
    const uint32_t tile = static_cast<uint32_t>(atoi(argv[3])), unit = static_cast<uint32_t>(atoi(argv[4]));
    if (tile < 64 || tile % 64 || tile > kScMaxTile || unit < 64 || unit % 64) die("bad tile or unit");
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
        const uint32_t K = get32(in, &at), want_slots = get32(in, &at), flen = get32(in, &at);
        if (K < kScMinK || K > kScMaxK || at + flen > in.size()) die("bad case");
        const auto fasta = exact(in.data() + at, flen);
        at += flen;
        SetResult set;
        set.status = flen && fasta[0] != '>' ? 1u : 0u;
        build_pass(fasta.get(), flen, K, unit, false, &set);
        set.nslots = want_slots;
        if (!set.nslots)
            for (set.nslots = kScMinSlots; set.nslots < 2 * set.windows; set.nslots <<= 1) {}
        set.table.reset(new uint64_t[set.nslots]);
        for (uint64_t i = 0; i < set.nslots; ++i) set.table[i] = kScEmpty;
        build_pass(fasta.get(), flen, K, unit, true, &set);
        put(out, set.status);
        put(out, set.windows);
        put(out, set.distinct);
        put(out, set.nslots);
        std::vector<uint64_t> keys;
        for (uint64_t i = 0; i < set.nslots; ++i)
            if (set.table[i] != kScEmpty) keys.push_back(set.table[i]);
        std::sort(keys.begin(), keys.end());
        if (keys.size() != set.distinct) die("the slots won are not the slots held");
        for (uint64_t k : keys) put(out, k);
        const uint32_t nreads = get32(in, &at);
        for (uint32_t r = 0; r < nreads; ++r) {
            const uint32_t L = get32(in, &at);
            if (at + L > in.size()) die("bad read");
            const auto seq = exact(in.data() + at, L);
            at += L;
            put(out, read_hits(seq.get(), L, set, K, tile));
        }
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) die("cannot write OUT");
    fclose(f);
    return 0;
}
