// vk_tree.h -- `tree`: neighbour joining of a batch of distance matrices, one record of joins and branch lengths per
// matrix.  Part of the one translation unit vkimg.hip (device code for gfx950; see the notes there).
//
// The rule ("`tree`: the rule"; tests/tree_ref.py is the same rule in Python, twice).  All arithmetic is
// IEEE double, one operation at a time in the order written: every function that computes carries `#pragma clang fp
// contract(off)`, so no multiply is fused with an add whatever the build's flags say.  Slots 0 .. n - 1, all active at the
// start.  R[i] = sum of D[i][k] over active k != i, taken as 256 partial sums (partial p adds the entries with k % 256 ==
// p in rising k, from +0.0) folded by p[t] += p[t + s], s = 128 .. 1.  A step with m > 3 active slots joins the active
// pair i < j of the smallest Q = ((m - 2) D[i][j] - R[i]) - R[j] (ties: the smaller i, then the smaller j); Li = 0.5 D[i][j]
// + (R[i] - R[j]) / (2 (m - 2)), Lj = D[i][j] - Li; for every other active k, Du[k] = 0.5 ((D[i][k] + D[j][k]) - D[i][j])
// and R[k] = ((R[k] - D[i][k]) - D[j][k]) + Du[k]; Du becomes row and column i, slot j retires, R[i] is summed afresh.
// The last three slots a < b < c close the record with 0.5 ((Dab + Dac) - Dbc), 0.5 ((Dab + Dbc) - Dac), 0.5 ((Dac + Dbc)
// - Dab).
//
// Launch sequence of vk_tree_nj_device (nothing allocates, synchronises or reads a device value on the host; a step is two
// launches in stream order, no workgroup waits for another):
//   vk_tr_init_kernel      a workgroup per row and tree: the row's entries checked (finite, 0 .. 1e100, the diagonal 0, equal
//                          bit for bit to the column's), its R by the 256-partial rule; a bad entry sets the tree's status,
//                          and every later workgroup of that tree returns at once
//   vk_tr_search_kernel    per step; a workgroup per tile of 512 columns, strip of 16 rows and tree.  Only the upper
//                          triangle is read: a block wholly below the diagonal writes an empty partial and returns.  The
//                          strip's active rows are listed once (a retired row is never read); a lane holds two
//                          neighbouring columns and reads them with one 16-byte load per row, all 16 rows in flight; R of
//                          the tile's columns lies in LDS, a retired slot's R is -inf there and in memory (its Q is never
//                          formed).  Rows of an odd n start at odd multiples of 8 bytes: the lane's pair then begins one
//                          column earlier, so that every load is 16-byte aligned.  The workgroup's smallest (Q, i, j) by
//                          wave shuffles, one partial per workgroup
//   vk_tr_join_kernel      per step; a workgroup per tree folds the partials, writes the step's record, computes Du and
//                          the new R[k] (row i is written coalesced, column i strided), sums R[i] afresh with lane p
//                          holding partial p, retires j
//   vk_tr_close_kernel     a workgroup per tree: the three slots still active and their lengths
// Retired slots are skipped, never compacted away: the matrix keeps its n x n layout, so a step reads n / 2 columns of each
// of its m rows.
//
// The lane-local code (tr_entry_ok .. tr_close3) compiles for the host: tests/emul/tree_emul.cpp runs it against
// tests/tree_ref.py.
#ifndef VK_TREE_H
#define VK_TREE_H

#include <cstdint>

namespace {

constexpr uint32_t kTrMinLeaves = 3, kTrMaxLeaves = 16384, kTrMaxTrees = 4096;   // VK_TREE_* (vkimg.h)
constexpr uint32_t kTrBadValue = 1;
constexpr uint32_t kTrPartials = 256;
constexpr uint32_t kTrTile = 512;     // columns of a search workgroup: two per lane
constexpr uint32_t kTrStrip = 16;     // rows of a search workgroup, all in flight in a lane at once: a workgroup waits for memory
                                      // once (with 64 rows in batches of 8 a search of 1,024 leaves took 23 us, eight waits)
constexpr uint32_t kTrUnroll = kTrStrip;
constexpr uint32_t kTrNone = 0xFFFFFFFFu;
constexpr double kTrMaxEntry = 1e100;

struct TrBest {   // a candidate pair; the empty one is (+inf, kTrNone, kTrNone)
    double q;
    uint32_t i, j;
};

__device__ inline double tr_dead() { return -__builtin_inf(); }   // R of a retired slot (a live R is finite)
__device__ inline bool tr_alive(double r) { return r != tr_dead(); }
__device__ inline uint64_t tr_bits(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}
// finite, >= 0 and <= 1e100 (a NaN fails both comparisons)
__device__ inline bool tr_entry_ok(double v) { return v >= 0.0 && v <= kTrMaxEntry; }
__host__ __device__ inline uint32_t tr_record_len(uint32_t n) { return 2u * (n - 3u) + 3u; }

__device__ inline double tr_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ inline double tr_q(double m2, double d, double ri, double rj) {
#pragma clang fp contract(off)
    const double a = m2 * d;
    const double b = a - ri;
    return b - rj;
}
// of two candidates the smaller Q, then the smaller i, then the smaller j
__device__ inline bool tr_less(const TrBest& a, const TrBest& b) {
    return a.q < b.q || (a.q == b.q && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}
__device__ inline TrBest tr_empty() { return TrBest{__builtin_inf(), kTrNone, kTrNone}; }
__device__ inline void tr_lengths(double dij, double ri, double rj, double m2, double* li, double* lj) {
#pragma clang fp contract(off)
    const double half = 0.5 * dij;
    const double diff = ri - rj;
    const double den = 2.0 * m2;
    const double quot = diff / den;
    *li = half + quot;
    *lj = dij - *li;
}
__device__ inline double tr_du(double dik, double djk, double dij) {
#pragma clang fp contract(off)
    const double s = dik + djk;
    const double t = s - dij;
    return 0.5 * t;
}
__device__ inline double tr_rk(double rk, double dik, double djk, double du) {
#pragma clang fp contract(off)
    const double a = rk - dik;
    const double b = a - djk;
    return b + du;
}
__device__ inline void tr_close3(double dab, double dac, double dbc, double* out) {
    out[0] = tr_du(dab, dac, dbc);
    out[1] = tr_du(dab, dbc, dac);
    out[2] = tr_du(dac, dbc, dab);
}
// Row `row` of n entries begins at an even (a = 0) or odd (a = 1) multiple of 8 bytes; lane `lane` of the tile at column
// c0 then holds columns c and c + 1 with c = c0 + 2 lane - a (-1 for the first lane of the first tile of an odd row), a
// 16-byte aligned pair.  It loads when one of the two is a column j with i < j < n.
__device__ inline uint32_t tr_parity(const double* row) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row) >> 3) & 1u; }
__device__ inline int32_t tr_first_col(uint32_t c0, uint32_t lane, uint32_t a) { return static_cast<int32_t>(c0 + 2u * lane) - static_cast<int32_t>(a); }
__device__ inline bool tr_loads(int32_t c, uint32_t i, uint32_t n) { return c + 1 > static_cast<int32_t>(i) && c < static_cast<int32_t>(n); }
// One loaded value: column j of row i with R[j] = rj.  (A column at or past n has a dead R: the caller fills it so.)
__device__ inline void tr_consider(TrBest* best, double m2, double d, double ri, double rj, uint32_t i, int32_t j) {
    if (j > static_cast<int32_t>(i) && tr_alive(rj)) {
        const TrBest cand{tr_q(m2, d, ri, rj), i, static_cast<uint32_t>(j)};
        if (tr_less(cand, *best)) *best = cand;
    }
}

#ifndef VK_TREE_LANE_ONLY

static_assert(kTrPartials == kClThreads, "lane p holds partial p");
static_assert(kTrTile == 2 * kClThreads, "a lane holds two columns of the tile");
static_assert(kTrStrip <= 64, "one wave lists the strip's rows");

// s_p[t] += s_p[t + s] for s = 128 .. 1; every lane of the workgroup calls it, the sum is s_p[0] after it
__device__ inline void tr_fold(double* s_p) {
    __syncthreads();
    for (uint32_t s = kTrPartials / 2; s; s >>= 1) {
        if (threadIdx.x < s) s_p[threadIdx.x] = tr_add(s_p[threadIdx.x], s_p[threadIdx.x + s]);
        __syncthreads();
    }
}

// the workgroup's smallest candidate, in every lane
__device__ inline TrBest tr_block_min(TrBest best, TrBest* s_best) {
    for (uint32_t d = 32; d; d >>= 1) {
        TrBest o;
        o.q = __shfl_down(best.q, d, 64);
        o.i = __shfl_down(best.i, d, 64);
        o.j = __shfl_down(best.j, d, 64);
        if (tr_less(o, best)) best = o;
    }
    if ((threadIdx.x & 63u) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    best = s_best[0];
    for (uint32_t w = 1; w < kClThreads / 64; ++w)
        if (tr_less(s_best[w], best)) best = s_best[w];
    return best;
}

__global__ void __launch_bounds__(kClThreads) vk_tr_init_kernel(const double* dist, uint32_t n, double* Rall, uint32_t* status) {
    __shared__ double s_p[kTrPartials];
    __shared__ uint32_t s_bad;
    const uint32_t tree = blockIdx.y, i = blockIdx.x;
    const double* D = dist + static_cast<uint64_t>(tree) * n * n;
    const double* row = D + static_cast<uint64_t>(i) * n;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    double p = 0.0;
    bool bad = false;
    for (uint32_t k = threadIdx.x; k < n; k += kClThreads) {
        const double v = row[k];
        bad |= !tr_entry_ok(v) || tr_bits(v) != tr_bits(D[static_cast<uint64_t>(k) * n + i]) || (k == i && !(v == 0.0));
        if (k != i) p = tr_add(p, v);
    }
    if (bad) s_bad = 1;   // (every writer writes the same)
    s_p[threadIdx.x] = p;
    tr_fold(s_p);
    if (threadIdx.x == 0) {
        Rall[static_cast<uint64_t>(tree) * n + i] = s_p[0];
        if (s_bad) atomicOr(status + tree, kTrBadValue);
    }
}

// `safe`: 16 readable, 16-byte aligned bytes (the workspace's first): what a lane without a pair of its own loads
__global__ void __launch_bounds__(kClThreads) vk_tr_search_kernel(const double* dist, uint32_t n, uint32_t m, const double* Rall,
                                                                 const uint32_t* status, const double* safe, TrBest* partials) {
    __shared__ double s_r[kTrTile + 2];   // R of columns c0 - 1 .. c0 + kTrTile, dead where there is no such column
    __shared__ uint32_t s_rows[kTrStrip];
    __shared__ double s_rowr[kTrStrip];
    __shared__ uint32_t s_nrows;
    __shared__ TrBest s_best[kClThreads / 64];
    const uint32_t tile = blockIdx.x, strip = blockIdx.y, tree = blockIdx.z;
    if (status[tree] != 0) return;   // (uniform; the join returns as well, the partial is never read)
    TrBest* out = partials + (static_cast<uint64_t>(tree) * gridDim.y + strip) * gridDim.x + tile;
    const uint32_t r0 = strip * kTrStrip, r1 = r0 + kTrStrip < n - 1u ? r0 + kTrStrip : n - 1u;   // (the last row has no j > i)
    const uint32_t c0 = tile * kTrTile;
    const double* R = Rall + static_cast<uint64_t>(tree) * n;
    if (c0 + kTrTile <= r0 + 1u) {   // no column of the tile lies right of the strip's first row (uniform)
        if (threadIdx.x == 0) *out = tr_empty();
        return;
    }
    for (uint32_t t = threadIdx.x; t < kTrTile + 2u; t += kClThreads) {
        const uint32_t col = c0 + t - 1u;   // (wraps for column -1: no such column)
        s_r[t] = col < n ? R[col] : tr_dead();
    }
    if (threadIdx.x < 64u) {
        const uint32_t row = r0 + threadIdx.x;
        const double r = row < r1 ? R[row] : tr_dead();
        const bool live = tr_alive(r);
        const uint64_t B = __ballot(live);
        if (live) {
            const uint32_t at = static_cast<uint32_t>(__popcll(B & ((1ull << threadIdx.x) - 1ull)));
            s_rows[at] = row;
            s_rowr[at] = r;
        }
        if (threadIdx.x == 0) s_nrows = static_cast<uint32_t>(__popcll(B));
    }
    __syncthreads();
    const uint32_t nrows = s_nrows;
    if (nrows == 0) {   // (uniform)
        if (threadIdx.x == 0) *out = tr_empty();
        return;
    }
    const double* D = dist + static_cast<uint64_t>(tree) * n * n;
    const double m2 = static_cast<double>(m - 2u);
    TrBest best = tr_empty();
    for (uint32_t t0 = 0; t0 < nrows; t0 += kTrUnroll) {
        double2 v[kTrUnroll];
        int32_t col[kTrUnroll];
        uint32_t at[kTrUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kTrUnroll; ++u) {
            at[u] = t0 + u < nrows ? t0 + u : nrows - 1u;   // (past the list: its last row again, which changes no minimum)
            const uint32_t i = s_rows[at[u]];
            const double* row = D + static_cast<uint64_t>(i) * n;
            const uint32_t a = tr_parity(row);
            col[u] = tr_first_col(c0, threadIdx.x, a);
            // (col + 1 <= n for a lane that loads: the pair ends within row i + 1 at the latest, and i <= n - 2)
            const double* p = tr_loads(col[u], i, n) ? row + col[u] : safe;
            v[u] = *reinterpret_cast<const double2*>(p);
        }
#pragma unroll
        for (uint32_t u = 0; u < kTrUnroll; ++u) {
            const uint32_t i = s_rows[at[u]];
            if (!tr_loads(col[u], i, n)) continue;
            const double ri = s_rowr[at[u]];
            const uint32_t lds = static_cast<uint32_t>(col[u] + 1 - static_cast<int32_t>(c0));   // s_r's index of column col
            tr_consider(&best, m2, v[u].x, ri, s_r[lds], i, col[u]);
            tr_consider(&best, m2, v[u].y, ri, s_r[lds + 1u], i, col[u] + 1);
        }
    }
    best = tr_block_min(best, s_best);
    if (threadIdx.x == 0) *out = best;
}

__global__ void __launch_bounds__(kClThreads) vk_tr_join_kernel(double* dist, uint32_t n, uint32_t m, uint32_t step, double* Rall,
                                                               const uint32_t* status, const TrBest* partials, uint32_t nparts,
                                                               uint32_t* nodes, double* lengths) {
    __shared__ double s_p[kTrPartials];
    __shared__ TrBest s_best[kClThreads / 64];
    const uint32_t tree = blockIdx.x;
    if (status[tree] != 0) return;   // (uniform)
    const TrBest* parts = partials + static_cast<uint64_t>(tree) * nparts;
    TrBest best = tr_empty();
    for (uint32_t p = threadIdx.x; p < nparts; p += kClThreads)
        if (tr_less(parts[p], best)) best = parts[p];
    best = tr_block_min(best, s_best);
    const uint32_t i = best.i, j = best.j;
    if (i >= n || j >= n) return;   // (never for a valid matrix: m > 3 active slots always hold a pair; uniform)
    double* D = dist + static_cast<uint64_t>(tree) * n * n;
    double* R = Rall + static_cast<uint64_t>(tree) * n;
    double* rowi = D + static_cast<uint64_t>(i) * n;
    const double* rowj = D + static_cast<uint64_t>(j) * n;
    const double dij = rowi[j];
    double ri = 0.0, rj = 0.0;
    if (threadIdx.x == 0) {   // (the lane that replaces them below)
        ri = R[i];
        rj = R[j];
    }
    double p = 0.0;
    for (uint32_t k = threadIdx.x; k < n; k += kClThreads) {   // (lane p meets k % 256 == p in rising k)
        if (k == i || k == j) continue;
        const double rk = R[k];
        if (!tr_alive(rk)) continue;
        const double dik = rowi[k], djk = rowj[k];
        const double du = tr_du(dik, djk, dij);
        R[k] = tr_rk(rk, dik, djk, du);
        rowi[k] = du;
        D[static_cast<uint64_t>(k) * n + i] = du;
        p = tr_add(p, du);
    }
    s_p[threadIdx.x] = p;
    tr_fold(s_p);
    if (threadIdx.x == 0) {
        const uint64_t rec = static_cast<uint64_t>(tree) * tr_record_len(n) + 2ull * step;
        double li, lj;
        tr_lengths(dij, ri, rj, static_cast<double>(m - 2u), &li, &lj);
        nodes[rec] = i;
        nodes[rec + 1] = j;
        lengths[rec] = li;
        lengths[rec + 1] = lj;
        R[i] = s_p[0];
        R[j] = tr_dead();
    }
}

__global__ void __launch_bounds__(kClThreads) vk_tr_close_kernel(const double* dist, uint32_t n, const double* Rall,
                                                                const uint32_t* status, uint32_t* nodes, double* lengths) {
    __shared__ uint32_t s_slots[3];
    __shared__ uint32_t s_n;
    const uint32_t tree = blockIdx.x;
    if (status[tree] != 0) return;   // (uniform)
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const double* R = Rall + static_cast<uint64_t>(tree) * n;
    for (uint32_t k = threadIdx.x; k < n; k += kClThreads) {
        if (!tr_alive(R[k])) continue;
        const uint32_t at = atomicAdd(&s_n, 1u);
        if (at < 3u) s_slots[at] = k;
    }
    __syncthreads();
    if (threadIdx.x != 0 || s_n != 3u) return;
    uint32_t a = s_slots[0], b = s_slots[1], c = s_slots[2], t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
    const double* D = dist + static_cast<uint64_t>(tree) * n * n;
    const double dab = D[static_cast<uint64_t>(a) * n + b], dac = D[static_cast<uint64_t>(a) * n + c], dbc = D[static_cast<uint64_t>(b) * n + c];
    const uint64_t rec = static_cast<uint64_t>(tree) * tr_record_len(n) + 2ull * (n - 3u);
    double out[3];
    tr_close3(dab, dac, dbc, out);
    nodes[rec] = a;
    nodes[rec + 1] = b;
    nodes[rec + 2] = c;
    lengths[rec] = out[0];
    lengths[rec + 1] = out[1];
    lengths[rec + 2] = out[2];
}

#endif  // VK_TREE_LANE_ONLY

}  // namespace

#endif  // VK_TREE_H
