// slam_step.h -- what slam_step.hip (the kernel) and api_slam.hip (host side) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rgbdfe.h"

namespace rgbdfe {

// one pair of a step as the inlier-statistics kernel sees it: the slots of the newer and the older node and the host's
// decision.  (The decision travels with the two slot indices: the batch's own pair list does not outlive the batch.)
struct SlamStatsPair {
  uint32_t q_slot, t_slot;
  uint32_t accept;
};

// stats: [slot][stride] bytes, stride a multiple of 4 >= max_kp.  Returns the number of kernel launches.
int launch_inlier_stats(const rgbdfe_match_result* recs, const SlamStatsPair* pairs, uint32_t n, uint8_t* stats,
                        uint32_t stride, uint32_t max_kp, hipStream_t stream);

}  // namespace rgbdfe
