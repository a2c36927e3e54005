// adapter_emul.cpp -- CPU emulation of the lane-local device code of adapters by sequence (test only).
//
// Compiles the product's own csrc/vk_adapter.h for the host and runs, as they are:
//   cl_trim_seq           on one read and one adapter, the adapter packed the way vkimg.hip's ad_pack packs it
//   ad_key_ok             over all 4^10 keys
//   vk_ad_hist_kernel     one lane after another over a record index built here, the atomics as plain additions
//   vk_ad_collect_kernel  in the same way
// so that the CPU suite can hold their arithmetic -- window shifts and masks, the key filters, the counted positions
// and an occurrence's reaches -- against tests/adapter_ref.py without a GPU.
//
// What it does NOT cover:
//   - vk_ad_top_kernel and vk_ad_extend_kernel hold barriers (ad_block_reduce, the votes in LDS).  They compile here
//     but are never called: one lane after another cannot run them.
//   - ad_pack, ad_candidates, ad_detected and ad_accept live in vkimg.hip, which is not compiled here: ad_pack is
//     restated below (pack), the other three are not reached.
//   - ClAdapter, ClRec, cl_acgt, cl_rec_ok, cl_find_u64 and kClThreads are this file's restatements of vk_clean.h's
//     (kept out by its include guard), and the record index is rebuilt here from the text's newlines: a change to those
//     in vk_clean.h or vkimg.hip does not reach this file.
// Only the GPU tests (tests/test_gpu_adapter_edges.py, tests/test_gpu_adapters.py) run the real ones.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// what vk_adapter.h takes from the HIP headers (stub/hip/hip_runtime.h is empty) and from vk_clean.h
#define VK_CLEAN_H
#define __device__
#define __global__
#define __shared__ static
#define __launch_bounds__(...)
struct EmulDim { uint32_t x; };
static EmulDim threadIdx, blockIdx, blockDim;
using std::max;
using std::min;
template <typename T>
static inline T atomicAdd(T* p, T v) {
    const T old = *p;
    *p = old + v;
    return old;
}
static inline void __syncthreads() {}
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }

namespace {

constexpr uint32_t kClThreads = 256;
constexpr uint32_t kClMaxAdapter = 64;

struct ClAdapter {
    uint64_t lo, hi, nlo, nhi;
    uint32_t len, pad;
    uint8_t seq[kClMaxAdapter];
};

struct ClRec { uint64_t h, he, se, pe, qe; };

inline bool cl_acgt(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T'; }

inline bool cl_rec_ok(const uint8_t* text, const ClRec& r) {
    const uint64_t bad = ~0ull;
    if (r.h == bad || r.he == bad || r.se == bad || r.pe == bad || r.qe == bad) return false;
    if (!(r.h < r.he && r.he < r.se && r.se < r.pe && r.pe < r.qe)) return false;
    if (text[r.h] != '@' || text[r.se + 1] != '+') return false;
    return r.qe - r.pe == r.se - r.he;
}

inline uint32_t cl_find_u64(const uint64_t* base, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace

#include "vk_adapter.h"

namespace {

// vkimg.hip's ad_pack for one adapter
ClAdapter pack(const uint8_t* seq, uint32_t len) {
    ClAdapter d{};
    d.len = len;
    for (uint32_t i = 0; i < len; ++i) {
        const uint8_t b = seq[i];
        const uint64_t c = (b >> 1) & 3u, bad = (b == 'A' || b == 'C' || b == 'G' || b == 'T') ? 0u : 1u;
        d.seq[i] = b;
        (i < 32 ? d.lo : d.hi) |= c << (2 * (i % 32));
        (i < 32 ? d.nlo : d.nhi) |= bad << (2 * (i % 32));
    }
    return d;
}

// the record index as step B's newline passes leave it: every line end to its record, ~0 for one not seen
std::vector<ClRec> index_of(const uint8_t* text, uint64_t len) {
    std::vector<uint64_t> nls;
    for (uint64_t i = 0; i < len; ++i)
        if (text[i] == '\n') nls.push_back(i);
    const uint64_t nrec = nls.size() / 4;
    std::vector<ClRec> recs(nrec + 1, ClRec{~0ull, ~0ull, ~0ull, ~0ull, ~0ull});
    if (nrec) recs[0].h = 0;
    for (uint64_t l = 0; l < 4 * nrec; ++l) {
        ClRec& r = recs[l / 4];
        switch (l & 3) {
            case 0: r.he = nls[l]; break;
            case 1: r.se = nls[l]; break;
            case 2: r.pe = nls[l]; break;
            default:
                r.qe = nls[l];
                if (l / 4 + 1 < nrec) recs[l / 4 + 1].h = nls[l] + 1;
        }
    }
    return recs;
}

// the groups of a slice: group k is the next group_n[k] records of the text
struct Slice {
    std::vector<ClRec> recs;
    std::vector<AdGroup> groups;
    std::vector<uint64_t> base;
};

bool slice_of(const uint8_t* text, uint64_t len, const uint64_t* group_n, uint32_t ng, Slice* s) {
    s->recs = index_of(text, len);
    s->groups.resize(ng);
    s->base.assign(ng + 1ull, 0);
    uint64_t at = 0;
    for (uint32_t k = 0; k < ng; ++k) {
        s->groups[k] = AdGroup{at, group_n[k]};
        at += group_n[k];
        s->base[k + 1] = s->base[k] + group_n[k];
    }
    return at + 1 == s->recs.size();
}

template <typename F>
void every_lane(uint64_t nrec, F f) {   // the launch of vk_clean_detect_device: whole workgroups of kClThreads
    blockDim.x = kClThreads;
    for (uint64_t b = 0; b * kClThreads < nrec; ++b)
        for (uint32_t t = 0; t < kClThreads; ++t) {
            blockIdx.x = static_cast<uint32_t>(b);
            threadIdx.x = t;
            f();
        }
}

}  // namespace

// the read's new length; the read and the adapter are copied into buffers of their exact sizes first, so that a
// sanitizer sees every byte read past either
extern "C" uint32_t emul_trim_seq(const uint8_t* read, uint32_t rlen, const uint8_t* adapter, uint32_t alen) {
    if (alen == 0 || alen > kClMaxAdapter) return ~0u;
    std::vector<uint8_t> p(read, read + rlen);
    const ClAdapter ad = pack(adapter, alen);
    return cl_trim_seq(p.data(), rlen, &ad);
}

extern "C" void emul_key_ok(uint8_t* ok) {
    for (uint32_t key = 0; key < kAdKeys; ++key) ok[key] = ad_key_ok(key) ? 1 : 0;
}

// hist[k * 4^10 + key] of the text's groups; 1: group_n does not add up to the text's records
extern "C" int emul_hist(const uint8_t* text, uint64_t len, const uint64_t* group_n, uint32_t ng, uint32_t* hist) {
    Slice s;
    if (ng == 0 || !slice_of(text, len, group_n, ng, &s)) return 1;
    std::fill(hist, hist + static_cast<uint64_t>(ng) * kAdKeys, 0u);
    every_lane(s.base[ng], [&] { vk_ad_hist_kernel(text, s.recs.data(), s.groups.data(), s.base.data(), ng, hist); });
    return 0;
}

// The occurrences of the groups' candidates: keys / caps[k * 10 + c] as ad_candidates states them (cap 0: none), the
// lists one behind the other in that order.  counts[k * 10 + c] as the kernel leaves them; at / fwd / back hold the
// lists (sum of caps entries each).
extern "C" int emul_collect(const uint8_t* text, uint64_t len, const uint64_t* group_n, uint32_t ng, const uint32_t* keys,
                            const uint32_t* caps, uint32_t shift_tail, uint32_t* counts, uint64_t* at, uint32_t* fwd,
                            uint32_t* back) {
    Slice s;
    if (ng == 0 || !slice_of(text, len, group_n, ng, &s)) return 1;
    std::vector<AdCand> cands(static_cast<size_t>(ng) * kAdTop);
    uint64_t nocc = 0;
    for (size_t i = 0; i < cands.size(); ++i) {
        cands[i] = AdCand{keys[i], caps[i], nocc};
        nocc += caps[i];
    }
    std::vector<AdOcc> occ(nocc + 1, AdOcc{~0ull, ~0u, ~0u});
    std::fill(counts, counts + cands.size(), 0u);
    every_lane(s.base[ng], [&] {
        vk_ad_collect_kernel(text, s.recs.data(), s.groups.data(), s.base.data(), ng, cands.data(), shift_tail, counts,
                             occ.data());
    });
    for (uint64_t i = 0; i < nocc; ++i) {
        at[i] = occ[i].at;
        fwd[i] = occ[i].fwd;
        back[i] = occ[i].back;
    }
    return occ[nocc].at == ~0ull ? 0 : 2;   // (2: a write behind the lists)
}

#ifdef ADAPTER_EMUL_MAIN
// adapter_emul_san IN OUT: IN holds cases (u32 read length, u32 adapter length, the read, the adapter); OUT gets one
// u32 per case, cl_trim_seq's answer
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t hdr[2];
    while (fread(hdr, 4, 2, f) == 2) {
        std::vector<uint8_t> read(hdr[0]), ad(hdr[1]);
        if (hdr[0] && fread(read.data(), 1, hdr[0], f) != hdr[0]) return 3;
        if (hdr[1] && fread(ad.data(), 1, hdr[1], f) != hdr[1]) return 3;
        const uint32_t n = emul_trim_seq(read.data(), hdr[0], ad.data(), hdr[1]);
        fwrite(&n, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 3 : 0;
}
#endif
