// ingest.hip -- sensor-frame ingest, gfx950: the listener's and Node::Node's image preparation in one streaming kernel.
//
//   depth smaller / larger than the colour image -> cv::resize(INTER_NEAREST)   (src/openni_listener.cpp:651-655)
//   depthToCV8UC1: mask from depth, 16UC1 -> float metres                        (src/misc.cpp:414-430)
//   cv::cvtColor(visual, gray, CV_RGB2GRAY) for CV_8UC3                          (src/node.cpp:139-144)
//
// The kernel reads the staged raw visual and depth bytes of all frames of a launch chain and writes the gray plane, the
// detection mask and (where something on the device reads it) the float depth plane, in the layouts the detect / describe
// chains already read.  A pure HBM stream: a lane owns 16 consecutive pixels of a row, every access of the vector
// instantiation is 16 bytes per lane (three loads of colour, four (f32) or two (u16) of depth, one store of gray, one of
// mask, four of depth).  No LDS, no scratch: every array below is indexed by constants once the loops are unrolled.
// The resampled-depth instantiation gathers the depth samples through the host-built index tables; widths that are not
// a multiple of 16 take the scalar instantiation.  The two float expressions are depth_convert.h's (shared with emm.hip).
#include "ingest.h"
#include "depth_convert.h"

namespace rgbdfe {

// OpenCV 3.3 RGB2Gray<uchar>: R2Y = 4899, G2Y = 9617, B2Y = 1868, yuv_shift = 14, on the channels as stored
__device__ __forceinline__ uint32_t rgb2gray_u8(uint32_t c0, uint32_t c1, uint32_t c2) {
  return (c0 * 4899u + c1 * 9617u + c2 * 1868u + 8192u) >> 14;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 255u; }

template <bool VEC, bool RESAMPLE>
__global__ __launch_bounds__(256) void ingest_kernel(const IngestParams p) {
  const int cpr = (p.W + 15) >> 4;  // 16-pixel chunks per row
  const uint32_t id = blockIdx.x * 256u + threadIdx.x;
  if (id >= (uint32_t)cpr * (uint32_t)p.H) return;
  const int y = (int)(id / (uint32_t)cpr);
  const int x0 = ((int)id - y * cpr) << 4;
  const int n = VEC ? 16 : min(16, p.W - x0);
  const size_t k = blockIdx.y;
  const uint8_t* __restrict__ fr = p.raw + k * p.frame_bytes;
  const size_t pix = (size_t)y * (size_t)p.W + (size_t)x0;

  // ---- gray (node.cpp:139-144)
  if (p.gray) {
    uint8_t* __restrict__ out = p.gray + k * p.gray_stride + pix;
    const uint8_t* __restrict__ v = fr + pix * (size_t)p.channels;
    if (VEC) {
      uint32_t g[4] = {0u, 0u, 0u, 0u};
      if (p.channels == 3) {
        const uint4* q = reinterpret_cast<const uint4*>(v);
        const uint4 a = q[0], b = q[1], c = q[2];
        const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int i = 0; i < 16; ++i)
          g[i >> 2] |= rgb2gray_u8(byte_of(w, 3 * i), byte_of(w, 3 * i + 1), byte_of(w, 3 * i + 2)) << ((i & 3) * 8);
      } else {
        const uint4 a = *reinterpret_cast<const uint4*>(v);
        g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w;
      }
      *reinterpret_cast<uint4*>(out) = make_uint4(g[0], g[1], g[2], g[3]);
    } else {
      for (int i = 0; i < n; ++i)
        out[i] = p.channels == 3 ? (uint8_t)rgb2gray_u8(v[3 * i], v[3 * i + 1], v[3 * i + 2]) : v[i];
    }
  }

  // ---- depth: nearest-neighbour resampling on the raw samples (openni_listener.cpp:651-655), then depthToCV8UC1
  if (!p.mask && !p.depth_m) return;
  const uint8_t* __restrict__ dimg = fr + p.depth_off;
  float d[16];     // metres
  uint32_t m[16];  // mask bytes
  if (RESAMPLE) {
    const size_t row = (size_t)p.ymap[y] * (size_t)p.dW;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      d[i] = 0.f; m[i] = 0u;
      if (i < n) {
        const size_t s = row + (size_t)p.xmap[x0 + i];
        if (p.depth_u16) {
          const float t = (float)reinterpret_cast<const uint16_t*>(dimg)[s];
          m[i] = depth_mm_to_mono8(t); d[i] = depth_mm_to_metres(t);
        } else {
          d[i] = reinterpret_cast<const float*>(dimg)[s];
          m[i] = depth_f32_to_mono8(d[i]);
        }
      }
    }
  } else if (VEC) {
    if (p.depth_u16) {
      const uint4* q = reinterpret_cast<const uint4*>(dimg + pix * 2);
      const uint4 a = q[0], b = q[1];
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float t = (float)((w[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu);
        m[i] = depth_mm_to_mono8(t); d[i] = depth_mm_to_metres(t);
      }
    } else {
      const float4* q = reinterpret_cast<const float4*>(dimg + pix * 4);
      const float4 a = q[0], b = q[1], c = q[2], e = q[3];
      const float w[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e.x, e.y, e.z, e.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) { d[i] = w[i]; m[i] = depth_f32_to_mono8(w[i]); }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      d[i] = 0.f; m[i] = 0u;
      if (i < n) {
        if (p.depth_u16) {
          const float t = (float)reinterpret_cast<const uint16_t*>(dimg)[pix + i];
          m[i] = depth_mm_to_mono8(t); d[i] = depth_mm_to_metres(t);
        } else {
          d[i] = reinterpret_cast<const float*>(dimg)[pix + i];
          m[i] = depth_f32_to_mono8(d[i]);
        }
      }
    }
  }
  if (p.mask) {
    uint8_t* __restrict__ out = p.mask + k * p.mask_stride + pix;
    if (VEC) {
      uint32_t g[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 16; ++i) g[i >> 2] |= m[i] << ((i & 3) * 8);
      *reinterpret_cast<uint4*>(out) = make_uint4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < n) out[i] = (uint8_t)m[i];
    }
  }
  if (p.depth_m) {
    float* __restrict__ out = p.depth_m + k * p.depth_stride + pix;
    if (VEC) {
      float4* o4 = reinterpret_cast<float4*>(out);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float4 t;
        t.x = d[4 * j]; t.y = d[4 * j + 1]; t.z = d[4 * j + 2]; t.w = d[4 * j + 3];
        o4[j] = t;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < n) out[i] = d[i];
    }
  }
}

void launch_ingest(const IngestParams& p, int n_frames, hipStream_t stream) {
  if (n_frames <= 0 || p.W <= 0 || p.H <= 0) return;
  const bool resample = p.xmap != nullptr;
  auto a16 = [](const void* q, size_t stride_bytes) { return (((uintptr_t)q | stride_bytes) & 15u) == 0; };
  const bool vec = (p.W % 16) == 0 && a16(p.raw, p.frame_bytes) && (p.depth_off & 15u) == 0 && a16(p.gray, p.gray_stride) &&
                   a16(p.mask, p.mask_stride) && a16(p.depth_m, p.depth_stride * 4);
  const unsigned lanes = (unsigned)((p.W + 15) / 16) * (unsigned)p.H;
  const dim3 grid((lanes + 255u) / 256u, (unsigned)n_frames), block(256);
  if (vec && !resample) hipLaunchKernelGGL((ingest_kernel<true, false>), grid, block, 0, stream, p);
  else if (vec) hipLaunchKernelGGL((ingest_kernel<true, true>), grid, block, 0, stream, p);
  else if (!resample) hipLaunchKernelGGL((ingest_kernel<false, false>), grid, block, 0, stream, p);
  else hipLaunchKernelGGL((ingest_kernel<false, true>), grid, block, 0, stream, p);
}

}  // namespace rgbdfe
