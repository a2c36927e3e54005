// sketch_emul.cpp -- CPU emulation of the lane-local device code of the sketches (test only).
//
// Compiles the product's own csrc/vk_sketch.h for the host (VK_SKETCH_LANE_ONLY, VK_SPECTRUM_LANE_ONLY and
// VK_SCREEN_LANE_ONLY: sk_eligible, sk_under, sk_digit, sk_bits, sk_shift, sk_candidate, sk_diag, sk_walk, sk_merge, and
// from vk_screen.h sc_mix) and runs a case the way the kernels cut it, a lane at a time:
//   a sketch: rounds of the radix select -- every slot's digit under the prefix (sk_eligible, sc_mix, sk_under, sk_digit)
//   into 2,048 bins, the crossing bin picked as vk_sk_pick_kernel picks it, until the candidates fit `cap` -- then the
//   compaction (sk_candidate) into a buffer of exactly cap hashes, runs of `run` hashes sorted, and levels of merges in
//   which a lane finds its diagonal (sk_diag) and merges its kSkMergePerLane values (sk_merge), ping-pong as
//   vk_sk_merge_kernel does;
//   a pair: 64 lanes, each its diagonal (sk_diag) and its segment (sk_walk), the scan of the distinct counts, and the
//   second walk of the lane where the count crosses `seen`, as vk_sk_pairs_kernel does.
// The keys, the counts, the buffers and the two sketches lie in heap blocks of exactly their size, so under the address
// sanitizer a read past a table, a sketch or a run is an error.
//
// What it does NOT cover: the kernels themselves -- the workgroups' cut of the slots, the LDS bins and their flush, the
// scan of vk_sk_pick_kernel, the wave-aggregated cursor of the compaction and the order it leaves, the bitonic sort of a
// run in LDS, the per-sample flags that end the rounds, the wave's scan and shuffles of the pairs: tests/test_gpu_sketch.py.
//
// A stand-alone program:  sketch_emul IN OUT
//   IN:  cases, each u32 kind.  kind 1 (sketch): u32 min_count, u32 s, u32 cap, u32 run, u64 nslots, u64 keys[nslots],
//        u32 counts[nslots].  kind 2 (pair): u32 s, u32 la, u32 lb, u64 A[la], u64 B[lb].
//   OUT: kind 1: u64 eligible, u64 length, u64 passes over the table, u64 hashes[length].  kind 2: u32 shared, u32 seen.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define __device__
#define __host__
inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long cmp, unsigned long long val) {
    const unsigned long long old = *p;
    if (old == cmp) *p = val;
    return old;
}
inline void sp_add(uint32_t* p, uint32_t n) { *p += n; }
#define VK_SCREEN_LANE_ONLY
#define VK_SPECTRUM_LANE_ONLY
#define VK_SKETCH_LANE_ONLY
#include "vk_sketch.h"

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "sketch_emul: %s\n", what);
    exit(2);
}

struct In {
    std::vector<uint8_t> bytes;
    size_t at = 0;
    template <class T> T get() {
        if (at + sizeof(T) > bytes.size()) die("short input");
        T v;
        memcpy(&v, bytes.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    template <class T> std::unique_ptr<T[]> block(size_t n) {   // a heap block of exactly n values
        std::unique_ptr<T[]> p(new T[n ? n : 1]);
        if (at + n * sizeof(T) > bytes.size()) die("short input");
        memcpy(p.get(), bytes.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return p;
    }
};

template <class T>
void put(std::vector<uint8_t>& out, T v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    out.insert(out.end(), p, p + sizeof(T));
}

void sketch_case(In& in, std::vector<uint8_t>& out) {
    const uint32_t m = in.get<uint32_t>(), s = in.get<uint32_t>(), cap = in.get<uint32_t>(), run = in.get<uint32_t>();
    const uint64_t nslots = in.get<uint64_t>();
    if (m < 1 || s < 1 || cap < s || run < kSkMergePerLane || run % kSkMergePerLane || cap % run) die("bad sketch case");
    const auto keys = in.block<uint64_t>(nslots);
    const auto counts = in.block<uint32_t>(nslots);
    // the selection: vk_sk_hist_kernel's lanes and vk_sk_pick_kernel's choice, round by round
    uint64_t prefix = 0, below = 0, eligible = 0, passes = 0;
    uint32_t mode = kSkAll, shift = 0;
    for (uint32_t round = 0; round < kSkRounds; ++round) {
        std::unique_ptr<uint32_t[]> bins(new uint32_t[kSkBins]());
        ++passes;
        for (uint64_t i = 0; i < nslots; ++i) {
            if (!sk_eligible(keys[i], counts[i], m)) continue;
            const uint64_t h = sc_mix(keys[i]);
            if (!sk_under(h, prefix, round)) continue;
            const uint32_t d = sk_digit(h, round);
            if (d >= (1u << sk_bits(round))) die("a digit past its bins");
            ++bins[d];
        }
        uint64_t total = 0;
        for (uint32_t b = 0; b < kSkBins; ++b) total += bins[b];
        if (round == 0) {
            eligible = total;
            if (total <= cap) break;   // kSkAll
        }
        const uint64_t need = s - below;
        if (need < 1 || total < need) die("the crossing bin is not in this round");
        uint64_t cum = 0;
        uint32_t d = 0;
        while (cum + bins[d] < need) cum += bins[d++];
        below += cum;
        prefix = (prefix << sk_bits(round)) | d;
        shift = sk_shift(round);
        const bool done = below + bins[d] <= cap, last = round + 1 == kSkRounds;
        mode = done || !last ? kSkUpTo : kSkStrict;
        if (done || last) break;
    }
    // the compaction, in slot order (the device's order is any: the sort makes it the same)
    std::unique_ptr<uint64_t[]> a(new uint64_t[cap]), b(new uint64_t[cap]);
    uint64_t cursor = 0;
    ++passes;
    for (uint64_t i = 0; i < nslots; ++i) {
        if (!sk_eligible(keys[i], counts[i], m)) continue;
        const uint64_t h = sc_mix(keys[i]);
        if (!sk_candidate(h, mode, shift, prefix)) continue;
        if (cursor >= cap) die("more candidates than the buffer holds");
        a[cursor++] = h;
    }
    const uint32_t n = static_cast<uint32_t>(cursor), npad = (n + run - 1) / run * run;
    for (uint32_t i = n; i < npad; ++i) a[i] = ~0ull;
    for (uint32_t r0 = 0; r0 < npad; r0 += run) std::sort(a.get() + r0, a.get() + r0 + run);
    uint64_t *src = a.get(), *dst = b.get();
    for (uint64_t width = run; width < cap; width *= 2) {   // (every level of the largest buffer, as the device runs them)
        for (uint32_t o0 = 0; o0 < npad; o0 += kSkMergePerLane) {   // a lane
            const uint32_t w = static_cast<uint32_t>(width), a0 = o0 / (2u * w) * (2u * w);
            const uint32_t la = npad - a0 < w ? npad - a0 : w, lb = npad - a0 - la < w ? npad - a0 - la : w;
            // (blocks of exactly the two runs: a read past either is the sanitizer's)
            std::unique_ptr<uint64_t[]> A(new uint64_t[la ? la : 1]), B(new uint64_t[lb ? lb : 1]);
            memcpy(A.get(), src + a0, la * 8ull);
            memcpy(B.get(), src + a0 + la, lb * 8ull);
            const uint32_t d = o0 - a0, i = sk_diag(A.get(), la, B.get(), lb, d);
            if (i > la || d - i > lb) die("a diagonal past a run");
            sk_merge(A.get(), la, B.get(), lb, i, d - i, kSkMergePerLane, dst + o0);
        }
        std::swap(src, dst);
    }
    const uint64_t length = std::min<uint64_t>(s, eligible);
    put(out, eligible);
    put(out, length);
    put(out, passes);
    for (uint64_t i = 0; i < length; ++i) put(out, i < n ? src[i] : prefix);
}

void pair_case(In& in, std::vector<uint8_t>& out) {
    const uint32_t s = in.get<uint32_t>(), la = in.get<uint32_t>(), lb = in.get<uint32_t>();
    if (la > s || lb > s) die("bad pair case");
    const auto A = in.block<uint64_t>(la);
    const auto B = in.block<uint64_t>(lb);
    const uint32_t n = la + lb, seg = (n + 63u) / 64u;
    uint32_t i0[64], d0[64], d1[64], distinct[64], dups[64], incl[64];
    for (uint32_t lane = 0; lane < 64; ++lane) {
        d0[lane] = std::min(lane * seg, n);
        d1[lane] = std::min(d0[lane] + seg, n);
        i0[lane] = sk_diag(A.get(), la, B.get(), lb, d0[lane]);
        if (i0[lane] > la || d0[lane] - i0[lane] > lb) die("a diagonal past a sketch");
        sk_walk(A.get(), la, B.get(), lb, i0[lane], d0[lane] - i0[lane], d1[lane] - d0[lane], 0, ~0ull, &distinct[lane], &dups[lane]);
        incl[lane] = distinct[lane] + (lane ? incl[lane - 1] : 0u);
    }
    const uint32_t all = incl[63], sn = std::min(all, s);
    uint32_t shared = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t excl = incl[lane] - distinct[lane];
        uint32_t mine = incl[lane] <= sn ? dups[lane] : 0u, again;
        if (excl <= sn && sn < incl[lane])
            sk_walk(A.get(), la, B.get(), lb, i0[lane], d0[lane] - i0[lane], d1[lane] - d0[lane], excl, sn, &again, &mine);
        shared += mine;
    }
    put(out, shared);
    put(out, sn);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: sketch_emul IN OUT");
    In in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) die("cannot read IN");
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) in.bytes.insert(in.bytes.end(), buf, buf + n);
        fclose(f);
    }
    std::vector<uint8_t> out;
    while (in.at < in.bytes.size()) {
        const uint32_t kind = in.get<uint32_t>();
        if (kind == 1) sketch_case(in, out);
        else if (kind == 2) pair_case(in, out);
        else die("bad case kind");
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) die("cannot write OUT");
    fclose(f);
    return 0;
}
