// tests/emu/device_layout_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program around csrc/device_layout.h, the layout
// type behind the host code's device scratch and staging, so that it can run under the host sanitizers on host memory
// (tests/test_device_layout_host.py).
//   device_layout_main layout SPEC...   SPEC = r<bytes> (a working block) or p<bytes> (an uploaded block, filled with its
//                                       1-based position in the list).  One line "block <off> <bytes>" per block, then
//                                       "total <bytes>", "written ok" and "staged <hex of the staging vector>".
//   device_layout_main sort N           "block" lines of keys[0], keys[1], idx[0], idx[1], hist, digits, then "total".
// Every block is written end to end into a malloc block of exactly the total: a block that reaches outside is a sanitizer
// report, one that overlaps another is "written: block <i> was overwritten".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "device_layout.h"

using namespace rgbdfe_host;

static int write_all(const DeviceLayout& lay, const std::vector<Block>& blocks) {
  for (const Block& b : blocks) printf("block %zu %zu\n", b.off, b.bytes);
  printf("total %zu\n", lay.total());
  // exactly the total on the heap (malloc(0) may return NULL: no block has a byte then)
  unsigned char* base = static_cast<unsigned char*>(malloc(lay.total()));
  if (!base && lay.total()) return 4;
  for (size_t i = 0; i < blocks.size(); ++i) {
    unsigned char* p = at<unsigned char>(base, blocks[i]);
    for (size_t k = 0; k < round256(blocks[i].bytes); ++k) p[k] = (unsigned char)(i + 1);  // the block and its padding
  }
  for (size_t i = 0; i < blocks.size(); ++i) {
    const unsigned char* p = at<unsigned char>(base, blocks[i]);
    for (size_t k = 0; k < round256(blocks[i].bytes); ++k)
      if (p[k] != (unsigned char)(i + 1)) {
        printf("written: block %zu was overwritten\n", i);
        free(base);
        return 0;
      }
  }
  free(base);
  printf("written ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  DeviceLayout lay;
  std::vector<Block> blocks;
  if (mode == "sort" && argc == 3) {
    const SortWorkspace w = sort_workspace(lay, (size_t)strtoull(argv[2], nullptr, 10));
    blocks = {w.keys[0], w.keys[1], w.idx[0], w.idx[1], w.hist, w.digits};
    return write_all(lay, blocks);
  }
  if (mode != "layout") return 2;
  for (int a = 2; a < argc; ++a) {
    const size_t bytes = (size_t)strtoull(argv[a] + 1, nullptr, 10);
    if (argv[a][0] == 'r') {
      blocks.push_back(lay.room(bytes));
    } else if (argv[a][0] == 'p') {
      // an exact-size source: a read past its end is a report
      unsigned char* src = static_cast<unsigned char*>(malloc(bytes));
      if (!src && bytes) return 4;
      if (bytes) memset(src, a - 1, bytes);
      blocks.push_back(lay.put(src, bytes));
      free(src);
    } else {
      return 2;
    }
  }
  const int rc = write_all(lay, blocks);
  printf("staged ");
  for (size_t k = 0; k < lay.staged_bytes(); ++k) printf("%02x", (unsigned char)lay.staged()[k]);
  printf("\n");
  return rc;
}
