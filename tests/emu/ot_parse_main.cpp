// tests/emu/ot_parse_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program around csrc/ot_parse.h, the host-side reader
// behind rgbdfe_octomap_read, so that the parser can run under the host sanitizers on hand-made files
// (tests/test_ot_parse_host.py).  Usage: ot_parse_main RES_TEXT FILE...   One line per file: "ok <leaves> <xor of the
// leaves' bytes as 16 hex digits>" or "refused: <message>".
#include <cstdio>

#include "ot_parse.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  for (int a = 2; a < argc; ++a) {
    std::vector<uint8_t> bytes;
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 3;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);
    std::vector<rgbdfe_octomap_leaf> leaves;
    std::string err;
    // an exact-size copy on the heap: a read past the end is a report, not a lucky hit in the vector's spare room
    uint8_t* exact = new uint8_t[bytes.size() ? bytes.size() : 1];
    if (!bytes.empty()) memcpy(exact, bytes.data(), bytes.size());
    const bool ok = rgbdfe::ot_parse(exact, bytes.size(), argv[1], &leaves, &err);
    delete[] exact;
    if (!ok) {
      printf("refused: %s\n", err.c_str());
      continue;
    }
    unsigned long long x[2] = {0, 0};
    for (size_t i = 0; i < leaves.size(); ++i) {
      unsigned long long w[2];
      memcpy(w, &leaves[i], 16);
      x[0] ^= w[0] * (2 * i + 1);
      x[1] ^= w[1] * (2 * i + 1);
    }
    printf("ok %zu %016llx\n", leaves.size(), x[0] ^ x[1]);
  }
  return 0;
}
