// tests/emu/emu_display_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over tests/emu/emu_display.cpp for a
// sanitizer build on the CPU (tests/test_emu_display_kernels.py builds it with -fsanitize=address,undefined and runs it).
// Every cloud and every output buffer is a heap block of exactly the needed size, so a read or a write of the kernel source
// outside a cloud, or behind the counted sizes, is reported.  Clouds of one row, one cell, a few cells and one full tile, every form, steps 1 and 3, two
// nodes per call (the same cloud twice), with and without transforms.
#include "emu_display.cpp"

#include <random>

int main() {
  std::mt19937 rng(5);
  std::uniform_real_distribution<float> u(0.f, 1.f);
  const int shapes[][2] = {{1, 7}, {2, 2}, {7, 9}, {33, 33}};
  const int forms[][2] = {{0, 1}, {1, 1}, {2, 1}, {2, 3}};
  float Ts[32] = {0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 1, 2, 3, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -3, 2, 1, 1};
  long total = 0;
  int call = 0;
  for (auto& sh : shapes) {
    const int h = sh[0], w = sh[1];
    std::vector<float> cloud((size_t)h * w * 4);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        float* p = cloud.data() + 4 * ((size_t)y * w + x);
        p[0] = 0.004f * x;
        p[1] = 0.004f * y;
        p[2] = 1.f + 0.002f * u(rng) + (u(rng) < 0.05f ? 0.5f : 0.f);
        p[3] = u(rng);
        if (u(rng) < 0.2f) p[2] = NAN;
        if (u(rng) < 0.02f) p[0] = p[1] = p[2] = 0.f;
      }
    for (auto& f : forms) {
      const float* ptr[2] = {cloud.data(), cloud.data()};
      const int32_t hw[4] = {h, w, h, w};
      int32_t types[2];
      int64_t totals[2], first[6];
      const float* T = (call++ & 1) ? Ts : nullptr;
      emu_display(2, ptr, hw, T, f[0], f[1], 0.0009, INFINITY, nullptr, 0, nullptr, 0, totals, first, types);
      std::vector<float> v((size_t)totals[0] * 4);
      std::vector<int64_t> s((size_t)totals[1] * 2);
      if (emu_display(2, ptr, hw, T, f[0], f[1], 0.0009, INFINITY, v.data(), totals[0], s.data(), totals[1], totals, first, types) < 0) {
        printf("the second call counted more than the first\n");
        return 1;
      }
      if (first[4] != totals[0] || first[2] * 2 != totals[0] || first[5] != totals[1]) {
        printf("offsets of the twice-listed cloud\n");
        return 1;
      }
      total += totals[0] + totals[1];
    }
  }
  printf("ok %ld\n", total);
  return 0;
}
