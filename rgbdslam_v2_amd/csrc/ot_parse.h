// ot_parse.h -- the host-side reader of an .ot file (AbstractOcTree::write / readData of a ColorOcTree) down to its leaves.
// Plain C++ with no device code and no state, so that a stand-alone program can exercise it (tests/emu/ot_parse_main.cpp).
// The format and the refusals: include/rgbdfe.h, "the tree of a leaf set" and rgbdfe_octomap_read.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rgbdfe.h"

namespace rgbdfe {

namespace ot_detail {

struct Walk {
  const uint8_t* p;
  size_t size, at;
  int64_t count;
  std::vector<rgbdfe_octomap_leaf>* leaves;
  std::string* err;
};

// the record at w.at is the node of `depth` whose cells start at key k; its subtree follows in pre-order
inline bool walk(Walk& w, int depth, uint32_t k0, uint32_t k1, uint32_t k2) {
  if (w.size - w.at < 8) {
    *w.err = "the file is truncated (a node record is missing)";
    return false;
  }
  const uint8_t* r = w.p + w.at;
  w.at += 8;
  ++w.count;
  const uint32_t mask = r[7];
  if (depth == 16) {
    if (mask != 0) {
      *w.err = "a node of depth 16 has children";
      return false;
    }
    rgbdfe_octomap_leaf l;
    memset(&l, 0, sizeof(l));
    l.key[0] = (uint16_t)k0; l.key[1] = (uint16_t)k1; l.key[2] = (uint16_t)k2;
    memcpy(&l.log_odds, r, 4);
    l.rgb[0] = r[4]; l.rgb[1] = r[5]; l.rgb[2] = r[6];
    w.leaves->push_back(l);
    return true;
  }
  if (mask == 0) {
    *w.err = "a node above depth 16 has no children (a pruned tree)";
    return false;
  }
  const uint32_t b = 15u - (uint32_t)depth;  // the key bit the children's index is taken from
  for (uint32_t i = 0; i < 8; ++i)
    if ((mask >> i) & 1u)
      if (!walk(w, depth + 1, k0 | ((i & 1u) << b), k1 | (((i >> 1) & 1u) << b), k2 | (((i >> 2) & 1u) << b))) return false;
  return true;
}

}  // namespace ot_detail

// the leaves of the file in `bytes` (inner values are ignored: they are a function of the leaves).  res_text: the
// map's resolution as printf %g, which the file's must equal as text.  false: *err says what was refused.
inline bool ot_parse(const uint8_t* bytes, size_t size, const char* res_text, std::vector<rgbdfe_octomap_leaf>* leaves,
                     std::string* err) {
  leaves->clear();
  size_t at = 0;
  auto next_line = [&](std::string* line) {
    if (at >= size) return false;
    const uint8_t* e = (const uint8_t*)memchr(bytes + at, '\n', size - at);
    if (!e) return false;
    line->assign((const char*)bytes + at, (size_t)(e - (bytes + at)));
    at = (size_t)(e - bytes) + 1;
    return true;
  };
  std::string line, id, res, size_text;
  if (!next_line(&line) || line.compare(0, 21, "# Octomap OcTree file") != 0) {
    *err = "the first line is not '# Octomap OcTree file'";
    return false;
  }
  bool data = false;
  while (next_line(&line)) {
    if (line == "data") {
      data = true;
      break;
    }
    if (line.empty() || line[0] == '#') continue;
    const size_t sp = line.find(' ');
    const std::string name = line.substr(0, sp), value = sp == std::string::npos ? "" : line.substr(sp + 1);
    if (name == "id") id = value;
    else if (name == "size") size_text = value;
    else if (name == "res") res = value;
    else {
      *err = "an unknown header line: " + name;
      return false;
    }
  }
  if (!data) {
    *err = "the file is truncated (no 'data' line)";
    return false;
  }
  if (id != "ColorOcTree") {
    *err = "the id is '" + id + "', not ColorOcTree";
    return false;
  }
  if (res != res_text) {
    *err = "the file's res is '" + res + "', the map's is '" + res_text + "'";
    return false;
  }
  char* end = nullptr;
  const unsigned long long n_nodes = strtoull(size_text.c_str(), &end, 10);
  if (size_text.empty() || *end != '\0' || size_text[0] < '0' || size_text[0] > '9') {
    *err = "the size line holds no number";
    return false;
  }
  ot_detail::Walk w{bytes + at, size - at, 0, 0, leaves, err};
  if (n_nodes > 0 && !ot_detail::walk(w, 0, 0, 0, 0)) {
    leaves->clear();
    return false;
  }
  if ((unsigned long long)w.count != n_nodes || w.at != w.size) {
    leaves->clear();
    *err = "the size line (" + size_text + ") does not match the records (" + std::to_string(w.count) + " in the tree, " +
           std::to_string(w.size - w.at) + " bytes behind it)";
    return false;
  }
  return true;
}

}  // namespace rgbdfe
