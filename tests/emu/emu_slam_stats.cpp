// tests/emu/emu_slam_stats.cpp -- TEST INFRASTRUCTURE ONLY: csrc/slam_step.hip compiled as host C++ over
// tests/emu/hip/hip_runtime.h (tests/test_emu_slam_stats_kernel.py builds it: the kernel SOURCE of the product runs, one OS
// thread per HIP thread, so the compare-and-swap loops of different lanes do race).
#include "hip/hip_runtime.h"

#include "hipemu_runtime.inc"

// the one atomic the kernel uses that the vocabulary does not have yet
static inline unsigned int atomicCAS(unsigned int* p, unsigned int expected, unsigned int desired) {
  __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST);
  return expected;
}

#include "slam_step.hip"

// stats: [n_slots][stride] bytes, updated in place.  Returns the kernel launches.
extern "C" int emu_slam_stats(const rgbdfe_match_result* recs, const uint32_t* q_slot, const uint32_t* t_slot,
                              const uint8_t* accept, uint32_t n, uint8_t* stats, uint32_t stride, uint32_t max_kp) {
  std::vector<rgbdfe::SlamStatsPair> pairs(n);
  for (uint32_t k = 0; k < n; ++k) pairs[k] = rgbdfe::SlamStatsPair{q_slot[k], t_slot[k], accept[k]};
  return rgbdfe::launch_inlier_stats(recs, pairs.data(), n, stats, stride, max_kp, nullptr);
}
