// tests/emu/emu_render_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program over tests/emu/emu_render.cpp for a
// sanitizer build on the CPU (tests/test_emu_render_kernels.py builds it with -fsanitize=address,undefined and runs it).
// Every image, the vertex rows, the strip records and the queue are heap blocks of exactly the needed size, so a read or a
// write of the kernel source outside them is reported.  A POINTS node, a TRIANGLES node whose stream ends on a left-over
// row, a strip node with records of 1, 2, 3 and 8 vertices and an empty node, with vertices that are NaN, behind the camera,
// far outside the guard band or in the image; cameras with w = 1 and with perspective; point sizes 1, 5 and 64; in one group
// and in a group per node, whose images must agree.
#include "emu_render.cpp"

#include <random>

int main() {
  std::mt19937 rng(11);
  std::uniform_real_distribution<float> u(0.f, 1.f);
  const int64_t counts[4] = {37, 3 * 9 + 1, 14, 0};
  const int32_t types[4] = {0, 1, 2, 1};
  int64_t off[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) off[k + 1] = off[k] + counts[k];
  const int64_t s0 = off[2];
  const std::vector<int64_t> strips = {s0, 1, s0 + 1, 2, s0 + 3, 3, s0 + 6, 8};
  const int64_t soff[5] = {0, 0, 0, 4, 4};
  const int32_t one_group[2] = {0, 4}, per_node[5] = {0, 1, 2, 3, 4};
  long total = 0;
  for (int round = 0; round < 6; ++round) {
    const int W = 17 + 5 * round, H = 12 + 3 * round;
    std::vector<float> v((size_t)off[4] * 4);
    for (size_t i = 0; i < v.size() / 4; ++i) {
      v[4 * i] = 4.f * u(rng) - 2.f;
      v[4 * i + 1] = 4.f * u(rng) - 2.f;
      v[4 * i + 2] = 1.f + u(rng);
      const uint32_t word = (uint32_t)(rng() & 0xffffffu);
      memcpy(&v[4 * i + 3], &word, 4);
      const float r = u(rng);
      if (r < 0.05f) v[4 * i + 2] = NAN;
      else if (r < 0.1f) v[4 * i + 2] = -1.f;
      else if (r < 0.15f) v[4 * i] = 1e30f;
      else if (r < 0.2f) v[4 * i + 1] = INFINITY;
    }
    double view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, proj[16] = {};
    if (round & 1) {  // perspective: w = z
      proj[0] = 0.7; proj[5] = -0.9; proj[10] = 1.2; proj[14] = -1.3; proj[11] = 1.0;
    } else {           // w = 1; round 4: a scale that sends most vertices past the guard band
      proj[0] = round == 4 ? 900.0 : 0.6; proj[5] = round == 4 ? -700.0 : -0.5; proj[10] = 0.9; proj[14] = -1.2; proj[15] = 1.0;
    }
    const int32_t point_n = round < 2 ? 1 : (round < 4 ? 5 : 64);
    const uint8_t clear[4] = {3, 3, 3, 3};
    const size_t np = (size_t)W * H;
    std::vector<uint8_t> rgba[2] = {std::vector<uint8_t>(4 * np), std::vector<uint8_t>(4 * np)};
    std::vector<float> depth[2] = {std::vector<float>(np), std::vector<float>(np)};
    std::vector<int64_t> ids[2] = {std::vector<int64_t>(np), std::vector<int64_t>(np)};
    std::vector<int32_t> node[2] = {std::vector<int32_t>(np), std::vector<int32_t>(np)};
    for (int pass = 0; pass < 2; ++pass) {
      const int rc = emu_render(4, v.data(), off, strips.data(), soff, types, pass ? 4 : 1, pass ? per_node : one_group, view, proj,
                                W, H, point_n, round & 2 ? 0 : 1, clear, rgba[pass].data(), depth[pass].data(), ids[pass].data(),
                                node[pass].data(), nullptr);
      if (rc < 0) {
        printf("a group left the queue non-empty\n");
        return 1;
      }
    }
    if (rgba[0] != rgba[1] || memcmp(depth[0].data(), depth[1].data(), 4 * np) != 0 || ids[0] != ids[1] || node[0] != node[1]) {
      printf("the images depend on the grouping (round %d)\n", round);
      return 1;
    }
    for (size_t p = 0; p < np; ++p) {
      const int64_t id = ids[0][p];
      if (id < -1 || id >= off[4] || (id < 0) != (node[0][p] < 0) || (id >= 0 && (id < off[node[0][p]] || id >= off[node[0][p] + 1]))) {
        printf("an id outside its node (round %d)\n", round);
        return 1;
      }
      total += id >= 0;
    }
  }
  printf("ok %ld\n", total);
  return 0;
}
