// tests/emu/cloud_file_main.cpp -- TEST INFRASTRUCTURE ONLY: csrc/cloud_file_format.h as a stand-alone host program
// (tests/test_cloud_file_format_host.py builds it with the address and undefined-behaviour sanitizers).  Per file named on
// the command line, one line:
//   ok <format> <width> <height> <points> <header bytes> <sum of the rows' bytes>     the parser accepted it and returned its rows
//   bad <cause>                                                                      the parser refused it
// The file's bytes are handed over in a heap block of exactly their length, and the rows are taken into a heap block of
// exactly 16 bytes per point, so that a read or a write past either end is the sanitizer's.  Every accepted file is also
// parsed as rgbdfe_cloud_file_info does it -- from its first kMaxHeaderBytes alone -- and must give the same header.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "cloud_file_format.h"

namespace cf = rgbdfe_cloud_file;

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> bytes;
    if (!read_file(argv[a], bytes)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
    std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes.size() ? bytes.size() : 1]);
    if (!bytes.empty()) memcpy(exact.get(), bytes.data(), bytes.size());
    rgbdfe_cloud_file_header info;
    std::string err = cf::parse_file(exact.get(), bytes.size(), info, nullptr);
    if (!err.empty()) { printf("bad %s\n", err.c_str()); continue; }
    std::unique_ptr<uint8_t[]> rows(new uint8_t[info.points ? cf::kRowBytes * (size_t)info.points : 1]);
    err = cf::parse_file(exact.get(), bytes.size(), info, rows.get());
    if (!err.empty()) { printf("bad %s\n", err.c_str()); continue; }
    const size_t head = bytes.size() < cf::kMaxHeaderBytes ? bytes.size() : cf::kMaxHeaderBytes;
    std::unique_ptr<uint8_t[]> prefix(new uint8_t[head ? head : 1]);
    memcpy(prefix.get(), exact.get(), head);
    rgbdfe_cloud_file_header again;
    err = cf::parse_header(prefix.get(), head, bytes.size(), again);
    if (!err.empty() || again.points != info.points || again.header_bytes != info.header_bytes || again.format != info.format) {
      printf("bad the header alone parses differently\n");
      continue;
    }
    unsigned long long sum = 0;
    for (size_t b = 0; b < cf::kRowBytes * (size_t)info.points; ++b) sum += rows[b];
    printf("ok %d %d %d %lld %lld %llu\n", info.format, info.width, info.height, (long long)info.points, (long long)info.header_bytes, sum);
  }
  return 0;
}
