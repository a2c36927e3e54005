// emit_emul.cpp -- CPU emulation of step C's file kernels (test only).
//
// Compiles the product's own csrc/vk_emit.h for the host: vk_em_status_kernel, vk_em_plan_kernel and
// vk_em_write_kernel run as they are, one lane after another (they hold no cross-lane operation and no barrier), around
// a record index stated here the way step B's newline passes leave it (csrc/vk_clean.h: every line end to its record,
// ~0 for one not seen) and the host's scan and 16-byte file layout of vk_ladder_emit_device.  Lets the CPU suite check
// the kernels' arithmetic -- record geometry, piece cuts and names, byte counts against bytes written -- against
// tests/ladder_emit_ref.py without a GPU.
//
// It checks vk_emit.h's arithmetic ONLY.  ClRec, cl_find_u64, cl_wave_copy and kClThreads below are this file's own
// restatements of vk_clean.h's (which needs the HIP headers and is kept out by its include guard), and the record index
// and the host's layout are rebuilt here: a change to those in vk_clean.h or vkimg.hip does not reach this file, and
// only the GPU tests (tests/test_gpu_ladder_emit.py) run the real ones.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

// what vk_emit.h takes from the HIP headers and from vk_clean.h
#define VK_CLEAN_H
#define __device__
#define __global__
#define __launch_bounds__(...)
#define VK_ST_BAD_START 1u
#define VK_ST_BAD_PHASE 2u
struct EmulDim { uint32_t x; };
static EmulDim threadIdx, blockIdx, blockDim;
using std::min;

namespace {

constexpr uint32_t kClThreads = 256;

struct ClRec { uint64_t h, he, se, pe, qe; };

inline uint32_t cl_find_u64(const uint64_t* base, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (base[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename F>
inline void cl_wave_copy(uint8_t* out, uint32_t n, uint32_t lane, F f) {
    for (uint32_t i = lane; i < n; i += 64) out[i] = f(i);
}

}  // namespace

#include "vk_emit.h"

// One sample, nsteps steps.  out_offsets / out_lengths / status as vk_ladder_emit_device gives them; returns 6
// (VK_ENOSPC) without writing when the files do not fit cap.
extern "C" int emul_emit(const uint8_t* text, uint64_t len, const uint64_t* seeds, const uint64_t* thresholds,
                         const uint8_t* whole, uint32_t nsteps, uint8_t* out, uint64_t cap, uint64_t* out_offsets,
                         uint64_t* out_lengths, uint32_t* status) {
    std::vector<uint64_t> nls;
    for (uint64_t i = 0; i < len; ++i)
        if (text[i] == '\n') nls.push_back(i);
    const uint64_t nrec = (nls.size() + 1) / 4;
    std::vector<ClRec> recs(nrec + 1, ClRec{~0ull, ~0ull, ~0ull, ~0ull, ~0ull});
    if (nrec) recs[0].h = 0;
    for (uint64_t l = 0; l < nls.size() && l < 4 * nrec; ++l) {
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
    const EmSample smp{0, len, 0, nrec, 0, 1};
    const uint64_t nl_prefix[2] = {0, nls.size()};
    blockDim.x = kClThreads;
    blockIdx.x = threadIdx.x = 0;
    vk_em_status_kernel(text, &smp, 1, recs.data(), nl_prefix, status);
    std::vector<EmStep> steps(nsteps);
    std::vector<uint64_t> base(nsteps + 1, 0);
    for (uint32_t j = 0; j < nsteps; ++j) {
        steps[j] = EmStep{seeds[j], thresholds[j], 0, 0, whole[j] ? 1u : 0u};
        base[j + 1] = base[j] + nrec;
    }
    const uint64_t nitems = base[nsteps];
    std::vector<uint64_t> bytes(nitems + 1, 0), prefix(nitems + 2, 0);
    for (uint64_t it = 0; it < nitems; ++it) {
        blockIdx.x = static_cast<uint32_t>(it / kClThreads);
        threadIdx.x = static_cast<uint32_t>(it % kClThreads);
        vk_em_plan_kernel(text, &smp, steps.data(), base.data(), nsteps, nitems, recs.data(), status, bytes.data());
    }
    for (uint64_t it = 0; it < nitems; ++it) prefix[it + 1] = prefix[it] + bytes[it];
    uint64_t at = 0;
    for (uint32_t j = 0; j < nsteps; ++j) {
        out_lengths[j] = prefix[base[j + 1]] - prefix[base[j]];
        out_offsets[j] = steps[j].out_off = at;
        at += (out_lengths[j] + 15) / 16 * 16;
    }
    if (at > cap) return 6;
    for (uint64_t b = 0; b * kEmItemsPerBlock < nitems; ++b)
        for (uint32_t t = 0; t < kClThreads; ++t) {
            blockIdx.x = static_cast<uint32_t>(b);
            threadIdx.x = t;
            vk_em_write_kernel(text, &smp, steps.data(), base.data(), nsteps, nitems, recs.data(), prefix.data(), out);
        }
    return 0;
}
