// vk_countplan.h -- the launch rule of the k <= 7 count whose workgroups pull their work (vk_count.h, vk_count_dense_kernel
// <K, false, true>).  Plain C++ over host values, shared by vkimg.hip and the host-only rule tests.
#ifndef VK_COUNTPLAN_H
#define VK_COUNTPLAN_H

#include <cstdint>

namespace {

// A sample's tickets for helpers where the device's share of workgroups per sample asks for fewer: what evens out the end
// of a launch of many samples, whose last owners would otherwise finish alone.
constexpr uint32_t kPullTailHelpers = 1;

struct PullPlan {
    uint32_t grid;      // workgroups of the launch; 0: this batch keeps the static launch
    uint32_t helpers;   // workgroups that may join a sample beside its owner: a sample is flushed 1 + helpers times at most
};

// `resident`: the workgroups the device holds at a time; `parts`: a sample's chunks / kWaves, the workgroups per sample of
// the static launch.
//  - samples of ONE part keep the static launch of a workgroup each (grid 0), unless a bound is forced: there is no flush to
//    save and nobody to help, and a claim per sample behind a barrier costs many small samples 17-23 % (600 x 20 KB: 0.097
//    against 0.115 ms; 4000 x 20 KB: 0.31 against 0.38).
//  - grid: what is resident, and never more than the static launch's nsamples * parts -- a workgroup's wavefronts want a
//    chunk each.
//  - helpers: the workgroups per sample beyond the owner when all of the grid works on the batch at once (32 samples on
//    512 workgroups: 15), kPullTailHelpers at least, and never more than the parts - 1 a sample can feed beside its owner
//    (a sample of one part is its owner's alone).  Bounded, so that the end of a launch does not come to a flush per chunk.
inline PullPlan pull_plan(uint32_t resident, uint32_t nsamples, uint32_t parts, uint32_t forced_helpers = 0xFFFFFFFFu) {
    PullPlan pl{0, 0};
    if (resident == 0 || nsamples == 0 || parts == 0) return pl;
    if (parts == 1 && forced_helpers == 0xFFFFFFFFu) return pl;
    const uint64_t units = static_cast<uint64_t>(nsamples) * parts;
    pl.grid = units < resident ? static_cast<uint32_t>(units) : resident;
    uint32_t h = (pl.grid + nsamples - 1) / nsamples - 1;
    if (h < kPullTailHelpers) h = kPullTailHelpers;
    if (forced_helpers != 0xFFFFFFFFu) h = forced_helpers;
    if (h > parts - 1) h = parts - 1;
    pl.helpers = h;
    return pl;
}

}  // namespace

#endif  // VK_COUNTPLAN_H
