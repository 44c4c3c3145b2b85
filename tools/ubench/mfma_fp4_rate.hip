// Micro-benchmark: what a stream of fp4 x fp4 MFMAs sustains on the box it runs on -- the ceiling the Hamming kernels' MFMA
// fraction is to be read against ("calibrate ... on the same box in the same call").  Both shapes of the
// instruction at the SAME output tile per wave: one 32x32x256 unit is a chain of 4 v_mfma_f32_32x32x64_f8f6f4 on one
// 16-register accumulator, or four chains of 2 v_mfma_f32_16x16x128_f8f6f4 on four 4-register accumulators.  A loop pass is two
// units: 2 x 16 accumulator registers against 8 x 4, what hamming_mfma.hip can hold.  For each shape:
//   * operands: "pm1" = every nibble +1.0 (0x2) or -1.0 (0xA), chosen per lane and register from a hash -- what the Hamming
//     kernels feed the unit; "trivial" = the operands this file used before (b: two registers zero, two 0.5), which cost the
//     unit less energy and so run at a higher clock: NOT the ceiling of a kernel on +-1 data;
//   * "bare": operands stay in registers; "lds": the train-side operand is re-read from LDS with ds_read_b128 at the kernels'
//     rate of 0.25 reads per large-MFMA equivalent (two reads per pass), one pass ahead of its use;
//   * 1 and 3 waves per SIMD, 256 CUs x 4 SIMDs.
// Prints one JSON line per case: TFLOP/s, the fraction of the 10 PFLOP/s dense fp4 figure, the clock the launch ran at
// (s_memrealtime is 100 MHz, s_memtime counts core cycles; one wave per block reports) and pipe cycles per MFMA per SIMD
// (launch time x clock over the MFMAs of a SIMD: the waves of a SIMD do not share the pipe evenly, the oldest runs ahead,
// so one wave's own cycle count says nothing at three waves; 32 / 16 = the issue rate of the large / small shape).
//   hipcc --offload-arch=gfx950 -O3 mfma_fp4_rate.hip -o mfma_fp4_rate && ./mfma_fp4_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ v8i op8(v4i v) {
  v8i o;
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
  o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;
  return o;
}
// register i of an operand: PM1 ? +-1.0 nibbles from a hash : the old trivial values
template <bool PM1>
__device__ __forceinline__ int a_word(uint32_t tid, int i, uint32_t salt) {
  return PM1 ? (int)(0x22222222u | (hash32(tid * 8u + (uint32_t)i + salt * 0x9E3779B9u) & 0x88888888u))
             : (int)(0x22222222u ^ (tid * 0x01010101u * (unsigned)i));
}
template <bool PM1>
__device__ __forceinline__ int b_word(uint32_t tid, int i) {
  return PM1 ? (int)(0x22222222u | (hash32(tid * 8u + (uint32_t)i + 0x51ED270Bu) & 0x88888888u)) : 0x11111111 * (i & 1);
}

template <int SHAPE, bool PM1, bool LDS>
__global__ __launch_bounds__(768) void k(float* out, uint64_t* cyc, int iters) {
  __shared__ uint4 img[8][256];   // eight 4 KB operand images ("train tiles"), read round robin
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  for (uint32_t p = tid; p < 8u * 256u; p += blockDim.x) {
    uint4 v;
    v.x = (uint32_t)a_word<PM1>(p, 0, 7u); v.y = (uint32_t)a_word<PM1>(p, 1, 7u);
    v.z = (uint32_t)a_word<PM1>(p, 2, 7u); v.w = (uint32_t)a_word<PM1>(p, 3, 7u);
    img[p >> 8][p & 255u] = v;
  }
  __syncthreads();
  v4i a0, a1, b;
  for (int i = 0; i < 4; ++i) { a0[i] = a_word<PM1>(tid, i, 1u); a1[i] = a_word<PM1>(tid, i, 2u); b[i] = b_word<PM1>(tid, i); }
  constexpr int NACC = SHAPE == 32 ? 2 : 8;
  v16f big[2];
  v4f small[8];
  for (int j = 0; j < 2; ++j)
    for (int i = 0; i < 16; ++i) big[j][i] = 0.f;
  for (int j = 0; j < 8; ++j)
    for (int i = 0; i < 4; ++i) small[j][i] = 0.f;
  const uint64_t c0 = __builtin_readcyclecounter();
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < iters; ++it) {
    v4i n0 = a0, n1 = a1;
    if (LDS) {   // the next pass's operands (a wave walks the images; two ds_read_b128 per pass)
      const uint4 x = img[it & 7][lane], y = img[(it + 3) & 7][128u + lane];
      n0[0] = (int)x.x; n0[1] = (int)x.y; n0[2] = (int)x.z; n0[3] = (int)x.w;
      n1[0] = (int)y.x; n1[1] = (int)y.y; n1[2] = (int)y.z; n1[3] = (int)y.w;
    }
    if (SHAPE == 32) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          big[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(op8(u & 1 ? a1 : a0), op8(b), big[j], 4, 4, 0, 0, 0, 0);
    } else {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          small[j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(op8(u & 1 ? a1 : a0), op8(b), small[j], 4, 4, 0, 0, 0, 0);
    }
    a0 = n0; a1 = n1;
  }
  const uint64_t c1 = __builtin_readcyclecounter();
  const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  float s = 0.f;
  for (int j = 0; j < 2; ++j)
    for (int i = 0; i < 16; ++i) s += big[j][i];
  for (int j = 0; j < 8; ++j)
    for (int i = 0; i < 4; ++i) s += small[j][i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (threadIdx.x == 0) { cyc[2 * blockIdx.x] = c1 - c0; cyc[2 * blockIdx.x + 1] = r1 - r0; }
  (void)NACC;
}

template <int SHAPE, bool PM1, bool LDS>
void run(int waves_per_simd, int cus) {
  const int iters = 6000;
  const int threads = 64 * 4 * waves_per_simd;
  float* out; uint64_t* cyc;
  hipMalloc(&out, (size_t)cus * threads * 4); hipMalloc(&cyc, (size_t)cus * 16);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipLaunchKernelGGL((k<SHAPE, PM1, LDS>), dim3(cus), dim3(threads), 0, 0, out, cyc, 50);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  hipLaunchKernelGGL((k<SHAPE, PM1, LDS>), dim3(cus), dim3(threads), 0, 0, out, cyc, iters);
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  std::vector<uint64_t> h((size_t)cus * 2); hipMemcpy(h.data(), cyc, (size_t)cus * 16, hipMemcpyDeviceToHost);
  double core = 0, real = 0; for (int i = 0; i < cus; ++i) { core += h[2 * i]; real += h[2 * i + 1]; }
  const int per_pass = SHAPE == 32 ? 8 : 16;   // MFMAs per loop pass (two 32x32x256 units)
  const double mfmas = (double)cus * 4 * waves_per_simd * iters * per_pass;
  const double flop = SHAPE == 32 ? 2.0 * 32 * 32 * 64 : 2.0 * 16 * 16 * 128;
  const double tflops = mfmas * flop / (ms * 1e-3) / 1e12;
  printf("{\"shape\": \"%s\", \"operands\": \"%s\", \"feed\": \"%s\", \"accumulators\": \"%s\", \"waves_per_simd\": %d, "
         "\"launch_ms\": %.3f, \"tflops\": %.1f, \"frac_of_10PF\": %.3f, \"core_clock_GHz\": %.3f, "
         "\"pipe_cycles_per_mfma_per_simd\": %.2f}\n",
         SHAPE == 32 ? "32x32x64" : "16x16x128", PM1 ? "pm1" : "trivial", LDS ? "lds" : "bare", SHAPE == 32 ? "2x16" : "8x4",
         waves_per_simd, ms, tflops, tflops / 10000.0, core / real / 10.0,
         ms * 1e-3 * (core / real * 1e8) / ((double)waves_per_simd * iters * per_pass));
  hipFree(out); hipFree(cyc);
}

template <bool PM1, bool LDS>
void both(int w, int cus) { run<32, PM1, LDS>(w, cus); run<16, PM1, LDS>(w, cus); }

int main() {
  int cus = 256;
  hipDeviceProp_t p; if (hipGetDeviceProperties(&p, 0) == hipSuccess && p.multiProcessorCount > 0) cus = p.multiProcessorCount;
  for (int rep = 0; rep < 2; ++rep)
    for (int w = 1; w <= 3; w += 2) {
      both<true, false>(w, cus); both<true, true>(w, cus);
      both<false, false>(w, cus); both<false, true>(w, cus);
    }
  return 0;
}
