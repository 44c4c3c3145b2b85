// cloud_file_format.h -- the bytes of the two point-cloud files the library writes and reads (include/rgbdfe.h, "map files"):
// binary PCD v0.7 with the fields `x y z rgb`, and binary little-endian PLY with 15-byte vertices and one camera record.
// Plain C++: no HIP headers, no device -- api_map_files.hip and tests/emu/cloud_file_main.cpp (under the sanitizers) include
// it.  The parser works on a byte range and a file length: it reads nothing outside the range, whatever the header claims.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rgbdfe.h"

namespace rgbdfe_cloud_file {

static_assert(sizeof(float) == 4, "IEEE-754 binary32");

constexpr int64_t kMaxPoints = ((int64_t)1 << 31) - 1;   // 2^31 points or more: RGBDFE_ERR_CAPACITY
constexpr size_t kRowBytes = 16, kPlyVertexBytes = 15, kPlyCameraBytes = 84;
constexpr size_t kMaxHeaderBytes = 2048;                 // both headers end well inside (a PCD's: 7 numbers of at most 15 characters)

// ---- the name rule (graph_mgr_io.cpp:555-563): *.ply in any letter case is PLY; anything else is PCD, and ".pcd" is appended
// unless the path ends in it in any case
inline bool ends_with_nocase(const std::string& s, const char* tail) {
  const size_t n = strlen(tail);
  if (s.size() < n) return false;
  for (size_t i = 0; i < n; ++i) {
    char c = s[s.size() - n + i];
    if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
    if (c != tail[i]) return false;
  }
  return true;
}
inline int32_t format_of_path(const std::string& path, std::string& final_path) {
  final_path = path;
  if (ends_with_nocase(path, ".ply")) return RGBDFE_CLOUD_FILE_PLY;
  if (!ends_with_nocase(path, ".pcd")) final_path += ".pcd";
  return RGBDFE_CLOUD_FILE_PCD;
}

// a float as a C++ stream prints it by default: printf("%g")
inline std::string fmt_g(float v) {
  char b[40];
  snprintf(b, sizeof(b), "%g", (double)v);
  return b;
}

// viewpoint: ox oy oz qw qx qy qz
inline std::string pcd_header(int64_t width, int64_t height, const float* viewpoint) {
  std::string h = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n";
  h += "WIDTH " + std::to_string(width) + "\nHEIGHT " + std::to_string(height) + "\nVIEWPOINT";
  for (int k = 0; k < 7; ++k) h += " " + fmt_g(viewpoint[k]);
  h += "\nPOINTS " + std::to_string(width * height) + "\nDATA binary\n";
  return h;
}

constexpr const char* kPlyHeadA = "ply\nformat binary_little_endian 1.0\ncomment PCL generated\nelement vertex ";
constexpr const char* kPlyHeadB =
    "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
    "element camera 1\nproperty float view_px\nproperty float view_py\nproperty float view_pz\nproperty float x_axisx\n"
    "property float x_axisy\nproperty float x_axisz\nproperty float y_axisx\nproperty float y_axisy\nproperty float y_axisz\n"
    "property float z_axisx\nproperty float z_axisy\nproperty float z_axisz\nproperty float focal\nproperty float scalex\n"
    "property float scaley\nproperty float centerx\nproperty float centery\nproperty int viewportx\nproperty int viewporty\n"
    "property float k1\nproperty float k2\nend_header\n";
inline std::string ply_header(int64_t n) { return std::string(kPlyHeadA) + std::to_string(n) + kPlyHeadB; }

// the camera record behind the vertices: origin, the identity row by row, five zero floats, the viewport, two zero floats
inline void ply_camera(int32_t width, int32_t height, uint8_t out[kPlyCameraBytes]) {
  float f[17] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0};
  memcpy(out, f, 68);
  memcpy(out + 68, &width, 4);
  memcpy(out + 72, &height, 4);
  memset(out + 76, 0, 8);
}

// n rows of 16 bytes -> n vertices of 15: x, y, z as they are, then bits 23-16, 15-8, 7-0 of the rgb word (what the device
// does in cloud_pack_ply_kernel, map_files.hip)
inline void ply_pack_rows(const uint8_t* rows, size_t n, uint8_t* out) {
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* r = rows + kRowBytes * i;
    uint8_t* v = out + kPlyVertexBytes * i;
    memcpy(v, r, 12);
    v[12] = r[14]; v[13] = r[13]; v[14] = r[12];
  }
}
// and back: the top byte of the rgb word is 0
inline void ply_unpack_rows(const uint8_t* vertices, size_t n, uint8_t* rows) {
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* v = vertices + kPlyVertexBytes * i;
    uint8_t* r = rows + kRowBytes * i;
    memcpy(r, v, 12);
    r[12] = v[14]; r[13] = v[13]; r[14] = v[12]; r[15] = 0;
  }
}

// ---- the parser -------------------------------------------------------------------------------------------------------
struct Cursor {
  const uint8_t* p;
  size_t n, at = 0;
  // the literal `s` at the cursor
  bool eat(const char* s) {
    const size_t k = strlen(s);
    if (n - at < k || memcmp(p + at, s, k) != 0) return false;
    at += k;
    return true;
  }
  // decimal digits (at least one, no sign, no leading blank) up to kMaxPoints
  bool count(int64_t& v) {
    size_t k = at;
    v = 0;
    while (k < n && p[k] >= '0' && p[k] <= '9') {
      v = v * 10 + (p[k] - '0');
      if (v > kMaxPoints) return false;
      ++k;
    }
    if (k == at) return false;
    at = k;
    return true;
  }
  // one number of a VIEWPOINT line: up to 31 characters that are neither blank nor newline, all of them consumed by strtof
  bool number(float& v) {
    char b[32];
    size_t k = 0;
    while (at + k < n && k < 31 && p[at + k] != ' ' && p[at + k] != '\n') { b[k] = (char)p[at + k]; ++k; }
    if (k == 0 || k == 31) return false;
    for (size_t i = 0; i < k; ++i)   // what %g prints, nothing strtof would take beyond it (hex floats, blanks)
      if (!strchr("0123456789+-.eEinfa", b[i])) return false;
    b[k] = 0;
    char* end = nullptr;
    v = strtof(b, &end);
    if (end != b + k) return false;
    at += k;
    return true;
  }
};

// The header in [p, p + n) of a file of file_bytes bytes (n <= file_bytes; n >= min(file_bytes, kMaxHeaderBytes) is enough).
// Returns "" and fills info, or the cause.  Accepted: exactly the two layouts of the contract, with a data section of exactly
// the promised length.
inline std::string parse_header(const uint8_t* p, size_t n, uint64_t file_bytes, rgbdfe_cloud_file_header& info) {
  memset(&info, 0, sizeof(info));
  Cursor c{p, n};
  if (c.eat("ply\n")) {
    c.at = 0;
    int64_t count = 0;
    if (!c.eat(kPlyHeadA) || !c.count(count)) return "cloud file: not the PLY header this library reads (element vertex)";
    if (!c.eat(kPlyHeadB)) return "cloud file: not the PLY header this library reads (properties, binary_little_endian, end_header)";
    info.format = RGBDFE_CLOUD_FILE_PLY;
    info.points = count;
    info.header_bytes = (int64_t)c.at;
    info.data_bytes = (int64_t)kPlyVertexBytes * count + (int64_t)kPlyCameraBytes;
    if (file_bytes - c.at != (uint64_t)info.data_bytes) return "cloud file: the PLY data section does not have the length the header promises";
    info.width = (int32_t)count;
    info.height = 1;
    info.viewpoint[3] = 1.0f;
    return "";
  }
  if (!c.eat("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n")) return "cloud file: neither a PCD v0.7 nor a PLY header";
  if (!c.eat("FIELDS x y z rgb\n")) return "cloud file: PCD fields other than x y z rgb";
  if (!c.eat("SIZE 4 4 4 4\n")) return "cloud file: PCD SIZE other than 4 4 4 4";
  if (!c.eat("TYPE F F F F\n")) return "cloud file: PCD TYPE other than F F F F";
  if (!c.eat("COUNT 1 1 1 1\n")) return "cloud file: PCD COUNT other than 1 1 1 1";
  int64_t w = 0, h = 0, points = 0;
  if (!c.eat("WIDTH ") || !c.count(w) || !c.eat("\nHEIGHT ") || !c.count(h) || !c.eat("\nVIEWPOINT"))
    return "cloud file: PCD WIDTH / HEIGHT are not counts below 2^31";
  for (int k = 0; k < 7; ++k)
    if (!c.eat(" ") || !c.number(info.viewpoint[k])) return "cloud file: PCD VIEWPOINT is not seven numbers";
  if (!c.eat("\nPOINTS ") || !c.count(points)) return "cloud file: PCD POINTS is not a count below 2^31";
  if (!c.eat("\nDATA binary\n")) return "cloud file: PCD DATA other than binary";
  if (w * h != points) return "cloud file: PCD POINTS is not WIDTH x HEIGHT";   // (both below 2^31: no overflow)
  info.format = RGBDFE_CLOUD_FILE_PCD;
  info.width = (int32_t)w;
  info.height = (int32_t)h;
  info.points = points;
  info.header_bytes = (int64_t)c.at;
  info.data_bytes = (int64_t)kRowBytes * points;
  if (file_bytes - c.at != (uint64_t)info.data_bytes) return "cloud file: the PCD data section does not have the length the header promises";
  return "";
}

// A PLY's camera record must be the one this library writes for the header's count (width x height == points is all a
// reader can hold it to: the viewport of an organised cloud is its own).  Fills width / height from it.
inline std::string parse_ply_camera(const uint8_t* cam, rgbdfe_cloud_file_header& info) {
  int32_t w = 0, h = 0;
  memcpy(&w, cam + 68, 4);
  memcpy(&h, cam + 72, 4);
  if (w < 0 || h < 0 || (int64_t)w * (int64_t)h != info.points) return "cloud file: the PLY camera's viewport is not width x height of the vertices";
  info.width = w;
  info.height = h;
  return "";
}

// A whole file in memory: header, lengths, then (out != NULL) the rows as 4 floats each into out[0 .. 16 * points).
inline std::string parse_file(const uint8_t* p, size_t n, rgbdfe_cloud_file_header& info, uint8_t* out) {
  std::string err = parse_header(p, n, n, info);
  if (!err.empty()) return err;
  const uint8_t* data = p + info.header_bytes;
  if (info.format == RGBDFE_CLOUD_FILE_PLY) {
    err = parse_ply_camera(data + kPlyVertexBytes * (size_t)info.points, info);
    if (!err.empty()) return err;
    if (out) ply_unpack_rows(data, (size_t)info.points, out);
  } else if (out && info.points) {
    memcpy(out, data, kRowBytes * (size_t)info.points);
  }
  return "";
}

}  // namespace rgbdfe_cloud_file
