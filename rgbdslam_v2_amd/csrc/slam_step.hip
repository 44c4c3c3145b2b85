// slam_step.hip -- updateInlierFeatures (graph_manager.cpp:409-419) for the accepted pairs of one SLAM step, from the
// result records the pair batch left in device memory: per accepted pair and set bit m of its inlier_mask,
// stats[new][all_q[m]] and stats[older][all_t[m]] go up by one and stop at 255.
//
// One wave per pair, a lane per match of a mask word (5 words: 320 matches).  The counters are bytes, four to a 32-bit
// word, and increments collide: a train row can be an inlier twice within a pair, a query row occurs in several accepted
// pairs of a step, and neighbouring rows of different pairs share a word.  Every increment is a compare-and-swap loop on
// the containing word that adds 1 to its byte unless the byte is 255, so none is lost and the result is the sequential
// loop's whatever the order (saturating addition commutes).  Integers only; a step has a few thousand increments at most,
// so contention is not worth a staging pass.
#include "slam_step.h"

namespace rgbdfe {

namespace {

__device__ inline void saturating_increment(uint8_t* stats, size_t byte_index) {
  unsigned int* word = reinterpret_cast<unsigned int*>(stats) + (byte_index >> 2);
  const unsigned int shift = (unsigned int)(byte_index & 3u) * 8u;
  unsigned int seen = *word;
  for (;;) {
    if (((seen >> shift) & 0xffu) == 0xffu) return;
    const unsigned int prev = atomicCAS(word, seen, seen + (1u << shift));
    if (prev == seen) return;
    seen = prev;
  }
}

__global__ __launch_bounds__(64) void inlier_stats_kernel(const rgbdfe_match_result* __restrict__ recs,
                                                          const SlamStatsPair* __restrict__ pairs, uint32_t n,
                                                          uint8_t* __restrict__ stats, uint32_t stride, uint32_t max_kp) {
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const SlamStatsPair p = pairs[k];
  if (!p.accept) return;
  const rgbdfe_match_result& r = recs[k];
  if (r.id1 < 0) return;
#pragma unroll
  for (int w = 0; w < RGBDFE_MASK_WORDS; ++w) {
    if (!((r.inlier_mask[w] >> lane) & 1ull)) continue;
    const uint32_t m = (uint32_t)w * 64u + lane;
    const uint32_t q = r.all_q[m], t = r.all_t[m];
    if (q < max_kp) saturating_increment(stats, (size_t)p.q_slot * stride + q);   // (rows beyond the slot: never written)
    if (t < max_kp) saturating_increment(stats, (size_t)p.t_slot * stride + t);
  }
}

}  // namespace

int launch_inlier_stats(const rgbdfe_match_result* recs, const SlamStatsPair* pairs, uint32_t n, uint8_t* stats,
                        uint32_t stride, uint32_t max_kp, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(inlier_stats_kernel, dim3(n), dim3(64), 0, stream, recs, pairs, n, stats, stride, max_kp);
  return 1;
}

}  // namespace rgbdfe
