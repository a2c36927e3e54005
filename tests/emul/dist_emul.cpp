// dist_emul.cpp -- CPU emulation of the host-compilable device code of `compare` (test only).
//
// Compiles the product's own csrc/vk_dist.h for the host (VK_DIST_HOST_ONLY: dist_padded, dist_strip_rows, dist_idx_bits,
// dist_key*, dist_fold, dist_prep_lane, dist_lane_min, dist_put and the constants) and runs a case the way vk_dist_device
// cuts it: every image prepared by 256 threads calling dist_prep_lane, the queries in strips of dist_strip_rows rows
// (VK_DIST_STRIP, a compile-time constant: the test builds this program at the product's value and at 64), an entry of a
// strip as |s|^2 + |t|^2 folded with the sum of every slice of kDistSlice pixels, a row's neighbours by 256 threads
// holding dist_lane_min's answer and only the winner's entries looked through again, a lane per 64th of them.  The
// matrix instruction is stood in by a plain loop over a slice's pixels of the prepared rows; its sum is checked to fit
// the i32 accumulator the kernel keeps it in.
// Every prepared row, norm table and strip lies in a heap block of exactly its size, so under the address sanitizer a
// byte touched past one is an error.
//
// What it does NOT cover: the tile kernel's staging, LDS layout and lane maps, the wave-wide sums and minima, the
// launches, VKIMG_DIST_STRIP: tests/test_gpu_dist.py.
//
// A stand-alone program:  dist_emul IN OUT
//   IN:  cases, each u32 nq, nr, npix, n, has_groups; q u8[nq][npix]; r u8[nr][npix]; with groups u32[nq], u32[nr].
//   OUT: per case the matrix u64[nq][nr], idx u32[nq][n], d2 u64[nq][n].
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define __device__
#define __host__
#define VK_DIST_HOST_ONLY
#include "vk_dist.h"

namespace {

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "dist_emul: %s\n", what);
    exit(2);
}

struct Prepared {
    std::unique_ptr<int8_t[]> rows;
    std::unique_ptr<uint64_t[]> norms;
};

Prepared prepare(const uint8_t* x, uint64_t n, uint64_t npix) {
    const uint64_t padded = dist_padded(npix);
    Prepared p{std::unique_ptr<int8_t[]>(new int8_t[n * padded]), std::unique_ptr<uint64_t[]>(new uint64_t[n])};
    for (uint64_t i = 0; i < n; ++i) {
        std::unique_ptr<uint8_t[]> img(new uint8_t[npix]);   // (a block of exactly the image's size)
        memcpy(img.get(), x + i * npix, npix);
        uint64_t sum = 0;
        for (uint32_t t = 0; t < kDistThreads; ++t) sum += dist_prep_lane(img.get(), p.rows.get() + i * padded, npix, padded, t, kDistThreads);
        p.norms[i] = sum;
    }
    return p;
}

void run_case(const uint8_t* q, const uint8_t* r, uint32_t nq, uint32_t nr, uint32_t npix, uint32_t nn, const uint32_t* qgroup,
              const uint32_t* rgroup, uint64_t* matrix, uint32_t* idx, uint64_t* d2) {
    if (nn < 1 || nn > kDistMaxN || nr > kDistMaxRefs || npix > kDistMaxPix) die("a case outside the limits");
    const uint32_t bits = dist_idx_bits(nr);
    if (!dist_key_fits(npix, bits)) die("a case whose keys do not fit");
    if ((1ull << bits) < nr || (bits > 1 && (1ull << (bits - 1)) >= nr)) die("dist_idx_bits");
    const uint64_t padded = dist_padded(npix);
    if (padded % kDistK || padded < npix || padded >= npix + kDistK) die("dist_padded");
    const Prepared Q = prepare(q, nq, npix), R = prepare(r, nr, npix);
    const uint64_t strip_rows = dist_strip_rows(nq, nr, VK_DIST_STRIP);
    if (strip_rows < 1 || strip_rows * nr * 8 > std::max<uint64_t>(kDistStripBytes, 8ull * kDistTile * nr)) die("dist_strip_rows");
    for (uint64_t q0 = 0; q0 < nq; q0 += strip_rows) {
        const uint32_t rows = static_cast<uint32_t>(std::min<uint64_t>(strip_rows, nq - q0));
        std::unique_ptr<uint64_t[]> strip(new uint64_t[static_cast<uint64_t>(rows) * nr]);
        for (uint32_t i = 0; i < rows; ++i)
            for (uint32_t j = 0; j < nr; ++j) {
                uint64_t* at = strip.get() + static_cast<uint64_t>(i) * nr + j;
                const int8_t *s = Q.rows.get() + (q0 + i) * padded, *t = R.rows.get() + static_cast<uint64_t>(j) * padded;
                for (uint64_t k0 = 0; k0 < padded; k0 += kDistSlice) {
                    const uint64_t k1 = std::min<uint64_t>(k0 + kDistSlice, padded);
                    int64_t acc = 0;   // (the matrix cores' sum over the slice)
                    for (uint64_t k = k0; k < k1; ++k) acc += static_cast<int64_t>(s[k]) * t[k];
                    if (acc > INT32_MAX || acc < INT32_MIN) die("a slice's sum does not fit an i32");
                    *at = dist_fold(k0 == 0 ? Q.norms[q0 + i] + R.norms[j] : *at, static_cast<int32_t>(acc));
                }
                matrix[(q0 + i) * nr + j] = *at;
                const uint64_t key = dist_key(*at, j, bits);
                if (key == kDistNoKey || dist_key_d2(key, bits) != *at || dist_key_idx(key, bits) != j) die("a key does not hold its halves");
            }
        for (uint32_t i = 0; i < rows; ++i) {
            const uint64_t* row = strip.get() + static_cast<uint64_t>(i) * nr;
            const uint32_t qg = qgroup ? qgroup[q0 + i] : kDistNoGroup;
            uint32_t* oi = idx + (q0 + i) * nn;
            uint64_t* od = d2 + (q0 + i) * nn;
            uint64_t mine[kDistSelThreads];
            for (uint32_t t = 0; t < kDistSelThreads; ++t) mine[t] = dist_lane_min(row, nr, rgroup, qg, bits, 0, false, t, kDistSelThreads);
            for (uint32_t rank = 0; rank < nn; ++rank) {
                const uint64_t best = *std::min_element(mine, mine + kDistSelThreads);
                dist_put(best, bits, oi + rank, od + rank);
                if (best == kDistNoKey) {
                    for (uint32_t f = rank + 1; f < nn; ++f) dist_put(kDistNoKey, bits, oi + f, od + f);
                    break;
                }
                for (uint32_t t = 0; t < kDistSelThreads; ++t) {
                    if (mine[t] != best) continue;
                    uint64_t next = kDistNoKey;   // (the owner's wavefront: lane x a 64th of its entries)
                    for (uint32_t x = 0; x < 64; ++x)
                        next = std::min(next, dist_lane_min(row, nr, rgroup, qg, bits, best, true, t + kDistSelThreads * x, kDistSelThreads * 64u));
                    mine[t] = next;
                }
            }
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: dist_emul IN OUT");
    std::vector<uint8_t> in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) die("cannot read IN");
        static uint8_t buf[1 << 20];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + n);
        fclose(f);
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) die("cannot write OUT");
    size_t at = 0;
    while (at < in.size()) {
        uint32_t h[5];
        if (at + sizeof h > in.size()) die("short input");
        memcpy(h, in.data() + at, sizeof h);
        at += sizeof h;
        const uint64_t nq = h[0], nr = h[1], npix = h[2], nn = h[3];
        const uint64_t need = (nq + nr) * npix + (h[4] ? 4 * (nq + nr) : 0);
        if (at + need > in.size()) die("bad case");
        // heap blocks of exactly the inputs' sizes
        std::unique_ptr<uint8_t[]> q(new uint8_t[nq * npix]), r(new uint8_t[nr * npix]);
        std::unique_ptr<uint32_t[]> qg(new uint32_t[nq]), rg(new uint32_t[nr]);
        memcpy(q.get(), in.data() + at, nq * npix);
        memcpy(r.get(), in.data() + at + nq * npix, nr * npix);
        at += (nq + nr) * npix;
        if (h[4]) {
            memcpy(qg.get(), in.data() + at, 4 * nq);
            memcpy(rg.get(), in.data() + at + 4 * nq, 4 * nr);
            at += 4 * (nq + nr);
        }
        std::vector<uint64_t> matrix(nq * nr), d2(nq * nn);
        std::vector<uint32_t> idx(nq * nn);
        run_case(q.get(), r.get(), h[0], h[1], h[2], h[3], h[4] ? qg.get() : nullptr, h[4] ? rg.get() : nullptr, matrix.data(),
                 idx.data(), d2.data());
        if (fwrite(matrix.data(), 8, matrix.size(), out) != matrix.size() || fwrite(idx.data(), 4, idx.size(), out) != idx.size() ||
            fwrite(d2.data(), 8, d2.size(), out) != d2.size())
            die("cannot write OUT");
    }
    fclose(out);
    return 0;
}
