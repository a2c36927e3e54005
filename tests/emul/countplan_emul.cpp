// Host build of the count launch's plan rule (csrc/vk_countplan.h) for the tests: tests/countplan_emul_lib.py.
#include "vk_countplan.h"

extern "C" {

// (grid, helpers) of a launch over `nsamples` samples of `parts` parts on a device that holds `resident` workgroups
void countplan_pull(uint32_t resident, uint32_t nsamples, uint32_t parts, uint32_t forced_helpers, uint32_t* out) {
    const PullPlan pl = pull_plan(resident, nsamples, parts, forced_helpers);
    out[0] = pl.grid;
    out[1] = pl.helpers;
}

uint32_t countplan_tail_helpers() { return kPullTailHelpers; }

}  // extern "C"
