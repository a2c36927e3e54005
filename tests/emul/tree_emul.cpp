// tree_emul.cpp -- CPU emulation of the lane-local device code of `tree` (test only).
//
// Compiles the product's own csrc/vk_tree.h (VK_TREE_LANE_ONLY: tr_entry_ok, tr_bits, tr_add, tr_q, tr_less, tr_lengths,
// tr_du, tr_rk, tr_close3, tr_parity, tr_first_col, tr_loads, tr_consider) and csrc/vk_sketch.h (VK_SKETCH_LANE_ONLY:
// sk_diag, sk_walk, sk_walk_blocks) for the host, with -ffp-contract=off, and runs a case the way the kernels cut it:
//   a tree: every row checked and summed as vk_tr_init_kernel's lanes do (lane p holds partial p, the fold by halves);
//   per step the search by tiles of 512 columns and strips of 16 rows -- the strip's active rows listed, every lane's
//   16-byte pair placed by the parity of the row's ADDRESS (the matrix can be laid at an odd multiple of 8 bytes, as
//   the second tree of an odd n lies on the device), both values of the pair read, each considered in the lane's own
//   order, the lanes' and then the workgroups' candidates folded with tr_less -- then the join's lanes (Du, R[k], the
//   partials of the new R[i], the lengths), and the closing three.
//   a pair: vk_sk_pair_blocks_kernel's 64 lanes, the scan of the distinct counts, the second walk into 2 x 64 counters.
// The matrix lies in a heap block of exactly its size (one double more in front when laid odd), so under the address
// sanitizer a pair read past its end is an error; a pair that begins before the matrix is refused here.
//
// What it does NOT cover: the kernels themselves -- the barriers and the LDS of the folds, the ballot that lists a
// strip's rows, the shuffles of the minimum, the order of the launches, the LDS atomics of the counters:
// tests/test_gpu_tree.py and tests/test_gpu_sketch_blocks.py.
//
// A stand-alone program:  tree_emul IN OUT
//   IN:  cases, each u32 kind.  kind 1 (tree): u32 n, u32 odd (0 or 1), f64 D[n][n].  kind 2 (pair): u32 s, u32 la,
//        u32 lb, u64 A[la], u64 B[lb].
//   OUT: kind 1: u32 status, u32 nodes[2 (n - 3) + 3], f64 lengths[2 (n - 3) + 3].  kind 2: u32 shared[64], u32 seen[64].
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
#define VK_TREE_LANE_ONLY
#include "vk_tree.h"

namespace {

constexpr uint32_t kLanes = 256;

[[noreturn]] void die(const char* what) {
    fprintf(stderr, "tree_emul: %s\n", what);
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
    template <class T> void read(T* p, size_t n) {
        if (at + n * sizeof(T) > bytes.size()) die("short input");
        memcpy(p, bytes.data() + at, n * sizeof(T));
        at += n * sizeof(T);
    }
};

template <class T>
void put(std::vector<uint8_t>& out, T v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    out.insert(out.end(), p, p + sizeof(T));
}

double fold(double* p) {   // tr_fold's halves
    for (uint32_t s = kTrPartials / 2; s; s >>= 1)
        for (uint32_t t = 0; t < s; ++t) p[t] = tr_add(p[t], p[t + s]);
    return p[0];
}

void tree_case(In& in, std::vector<uint8_t>& out) {
    const uint32_t n = in.get<uint32_t>(), odd = in.get<uint32_t>();
    if (n < kTrMinLeaves || n > 4096 || odd > 1) die("bad tree case");
    const size_t nn = static_cast<size_t>(n) * n;
    std::unique_ptr<double[]> block(new double[nn + odd]);   // (new[] of doubles is 16-byte aligned here: checked below)
    if (reinterpret_cast<uintptr_t>(block.get()) & 15u) die("a heap block that is not 16-byte aligned");
    double* D = block.get() + odd;
    in.read(D, nn);
    const uint32_t L = tr_record_len(n);
    std::vector<uint32_t> nodes(L, 0);
    std::vector<double> lengths(L, 0.0), R(n);
    // vk_tr_init_kernel: a workgroup per row
    bool bad = false;
    for (uint32_t i = 0; i < n; ++i) {
        double p[kTrPartials];
        for (uint32_t lane = 0; lane < kLanes; ++lane) {
            p[lane] = 0.0;
            for (uint32_t k = lane; k < n; k += kLanes) {
                const double v = D[static_cast<size_t>(i) * n + k];
                bad |= !tr_entry_ok(v) || tr_bits(v) != tr_bits(D[static_cast<size_t>(k) * n + i]) || (k == i && !(v == 0.0));
                if (k != i) p[lane] = tr_add(p[lane], v);
            }
        }
        R[i] = fold(p);
    }
    uint32_t status = bad ? kTrBadValue : 0;
    const uint32_t tiles = (n + kTrTile) / kTrTile, strips = (n - 1 + kTrStrip - 1) / kTrStrip;
    for (uint32_t step = 0; !bad && step + 3 < n; ++step) {
        const uint32_t m = n - step;
        const double m2 = static_cast<double>(m - 2u);
        // vk_tr_search_kernel: a workgroup per tile and strip; vk_tr_join_kernel folds their candidates
        TrBest all = tr_empty();
        for (uint32_t strip = 0; strip < strips; ++strip) {
            for (uint32_t tile = 0; tile < tiles; ++tile) {
                const uint32_t r0 = strip * kTrStrip, r1 = std::min(r0 + kTrStrip, n - 1u), c0 = tile * kTrTile;
                if (c0 + kTrTile <= r0 + 1u) continue;
                std::vector<double> s_r(kTrTile + 2);
                for (uint32_t t = 0; t < kTrTile + 2u; ++t) {
                    const uint32_t col = c0 + t - 1u;
                    s_r[t] = col < n ? R[col] : tr_dead();
                }
                std::vector<uint32_t> rows;
                for (uint32_t row = r0; row < r1; ++row)
                    if (tr_alive(R[row])) rows.push_back(row);
                TrBest wg = tr_empty();
                for (uint32_t lane = 0; lane < kLanes; ++lane) {
                    TrBest best = tr_empty();
                    for (uint32_t i : rows) {
                        const double* row = D + static_cast<size_t>(i) * n;
                        const int32_t col = tr_first_col(c0, lane, tr_parity(row));
                        if (!tr_loads(col, i, n)) continue;
                        if (col < 0 || (reinterpret_cast<uintptr_t>(row + col) & 15u)) die("a pair before the matrix, or not aligned");
                        const double v0 = row[col], v1 = row[col + 1];   // (the whole pair is read, as the device reads it)
                        const uint32_t lds = static_cast<uint32_t>(col + 1 - static_cast<int32_t>(c0));
                        if (lds + 1u >= kTrTile + 2u) die("a column past the tile's R");
                        tr_consider(&best, m2, v0, R[i], s_r[lds], i, col);
                        tr_consider(&best, m2, v1, R[i], s_r[lds + 1u], i, col + 1);
                    }
                    if (tr_less(best, wg)) wg = best;
                }
                if (tr_less(wg, all)) all = wg;
            }
        }
        const uint32_t i = all.i, j = all.j;
        if (i >= n || j >= n || i >= j) die("no pair found");
        // vk_tr_join_kernel
        const double dij = D[static_cast<size_t>(i) * n + j], ri = R[i], rj = R[j];
        double p[kTrPartials];
        for (uint32_t lane = 0; lane < kLanes; ++lane) {
            p[lane] = 0.0;
            for (uint32_t k = lane; k < n; k += kLanes) {
                if (k == i || k == j || !tr_alive(R[k])) continue;
                const double dik = D[static_cast<size_t>(i) * n + k], djk = D[static_cast<size_t>(j) * n + k];
                const double du = tr_du(dik, djk, dij);
                R[k] = tr_rk(R[k], dik, djk, du);
                D[static_cast<size_t>(i) * n + k] = du;
                D[static_cast<size_t>(k) * n + i] = du;
                p[lane] = tr_add(p[lane], du);
            }
        }
        tr_lengths(dij, ri, rj, m2, &lengths[2 * step], &lengths[2 * step + 1]);
        nodes[2 * step] = i;
        nodes[2 * step + 1] = j;
        R[i] = fold(p);
        R[j] = tr_dead();
    }
    if (!bad) {   // vk_tr_close_kernel
        std::vector<uint32_t> live;
        for (uint32_t k = 0; k < n; ++k)
            if (tr_alive(R[k])) live.push_back(k);
        if (live.size() != 3) die("not three slots at the end");
        const uint32_t a = live[0], b = live[1], c = live[2];
        tr_close3(D[static_cast<size_t>(a) * n + b], D[static_cast<size_t>(a) * n + c], D[static_cast<size_t>(b) * n + c], &lengths[L - 3]);
        nodes[L - 3] = a;
        nodes[L - 2] = b;
        nodes[L - 1] = c;
    }
    put(out, status);
    for (uint32_t x : nodes) put(out, x);
    for (double x : lengths) put(out, x);
}

void pair_case(In& in, std::vector<uint8_t>& out) {
    const uint32_t s = in.get<uint32_t>(), la = in.get<uint32_t>(), lb = in.get<uint32_t>();
    if (la > s || lb > s) die("bad pair case");
    std::unique_ptr<uint64_t[]> A(new uint64_t[la ? la : 1]), B(new uint64_t[lb ? lb : 1]);   // (of exactly their size)
    in.read(A.get(), la);
    in.read(B.get(), lb);
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
    const uint32_t sn = std::min(incl[63], s);
    uint32_t shared[kSkBlocks] = {}, seen[kSkBlocks] = {};
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t excl = incl[lane] - distinct[lane];
        if (excl <= sn)
            sk_walk_blocks(A.get(), la, B.get(), lb, i0[lane], d0[lane] - i0[lane], d1[lane] - d0[lane], excl, sn,
                           [&](uint64_t h) { ++seen[h & (kSkBlocks - 1u)]; }, [&](uint64_t h) { ++shared[h & (kSkBlocks - 1u)]; });
    }
    for (uint32_t x : shared) put(out, x);
    for (uint32_t x : seen) put(out, x);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) die("usage: tree_emul IN OUT");
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
        if (kind == 1) tree_case(in, out);
        else if (kind == 2) pair_case(in, out);
        else die("bad case kind");
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) die("cannot write OUT");
    fclose(f);
    return 0;
}
