#include "small_sweep.h"

#include <string.h>

namespace pt {

std::vector<float> SmallSweep::pack(bool hull_codes) const {
  const bool wide = n_boxes > 32;   // sweep_walk.h sweep_wide, sweep_need_words
  const size_t need_words = ((wide ? 2 : 1) * (size_t)n_leaves + 3) & ~(size_t)3;
  const size_t words = (size_t)8 * n_boxes + need_words + (size_t)n_leaves;
  std::vector<float> t((words + 3) / 4 * 4, 0.0f);
  if (n_boxes == 0) return t;
  memcpy(t.data(), boxes.data(), (size_t)8 * n_boxes * 4);
  for (int b = 1; b < n_boxes && !hull_codes; ++b) t[8 * (size_t)b + 7] = 0.0f;
  for (int l = 0; l < n_leaves; ++l) {
    const uint32_t w[2] = {(uint32_t)need[l], (uint32_t)(need[l] >> 32)};
    memcpy(t.data() + 8 * (size_t)n_boxes + (wide ? 2 : 1) * (size_t)l, w, wide ? 8 : 4);
  }
  memcpy(t.data() + 8 * (size_t)n_boxes + need_words, slot.data(), (size_t)n_leaves * 4);
  return t;
}

bool build_small_sweep(const float* collapsed, size_t n_kept, SmallSweep* out, int max_boxes, int max_leaves,
                       bool hull_codes) {
  *out = SmallSweep();
  if (n_kept == 0 || max_boxes > kSweepMaxBoxes || max_leaves > kSweepMaxLeaves) return false;
  auto skip_of = [&](size_t k) { int32_t s; memcpy(&s, collapsed + 8 * k + 3, 4); return (size_t)(s & 0x7fffffff); };
  auto tri_of = [&](size_t k) { int32_t t; memcpy(&t, collapsed + 8 * k + 7, 4); return t; };
  size_t leaves = 0;
  for (size_t k = 0; k < n_kept; ++k) leaves += tri_of(k) >= 0 ? 1 : 0;
  if (leaves > (size_t)max_leaves) return false;
  // distinct boxes by the 24 bytes of min/max, numbered by first appearance
  // (reordered by kind below): node 0 is the root, so its box is box 0.  An
  // implied leaf (kept, bit 31) has the box of a kept ancestor bitwise, hence
  // that ancestor's id.
  SmallSweep s;
  std::vector<int> box_id(n_kept);
  for (size_t k = 0; k < n_kept; ++k) {
    const float* nd = collapsed + 8 * k;
    int id = -1;
    for (int b = 0; b < s.n_boxes && id < 0; ++b)
      if (memcmp(&s.boxes[8 * (size_t)b], nd, 12) == 0 && memcmp(&s.boxes[8 * (size_t)b + 4], nd + 4, 12) == 0) id = b;
    if (id < 0) {
      if (s.n_boxes == max_boxes) return false;
      id = s.n_boxes++;
      const float rec[8] = {nd[0], nd[1], nd[2], 0.0f, nd[4], nd[5], nd[6], 0.0f};
      s.boxes.insert(s.boxes.end(), rec, rec + 8);
    }
    box_id[k] = id;
  }
  // order: root, general boxes, then the boxes flat (lo == hi bitwise) in x, y, z
  // (by their first flat axis); the four counts in the root record's last word
  {
    auto cls = [&](int b) {
      if (b == 0) return 0;
      for (int a = 0; a < 3; ++a)
        if (memcmp(&s.boxes[8 * (size_t)b + a], &s.boxes[8 * (size_t)b + 4 + a], 4) == 0) return 2 + a;
      return 1;
    };
    std::vector<int> new_id((size_t)s.n_boxes);
    std::vector<float> sorted;
    uint32_t counts[5] = {0, 0, 0, 0, 0};
    int next = 0;
    for (int c = 0; c < 5; ++c)
      for (int b = 0; b < s.n_boxes; ++b)
        if (cls(b) == c) {
          new_id[(size_t)b] = next++;
          ++counts[c];
          sorted.insert(sorted.end(), s.boxes.begin() + 8 * (size_t)b, s.boxes.begin() + 8 * (size_t)b + 8);
        }
    s.boxes = sorted;
    for (size_t k = 0; k < n_kept; ++k) box_id[k] = new_id[(size_t)box_id[k]];
    const uint32_t w = counts[1] | counts[2] << 8 | counts[3] << 16 | counts[4] << 24;
    memcpy(&s.boxes[7], &w, 4);
  }
  // hull faces: a flat box whose flat coordinate is bitwise the root's lo (code 1) or hi (code 2) on
  // that axis and whose other four extents are bitwise the root's; the code in the record's last word
  s.n_hull = 0;
  for (int b = 1; b < s.n_boxes && hull_codes; ++b) {
    float* r = &s.boxes[8 * (size_t)b];
    const float* r0 = &s.boxes[0];
    int flat = -1;
    for (int a = 2; a >= 0; --a)
      if (memcmp(r + a, r + 4 + a, 4) == 0) flat = a;   // the first flat axis, as cls above
    if (flat < 0) continue;
    bool same = true;
    for (int a = 0; a < 3; ++a)
      if (a != flat) same = same && memcmp(r + a, r0 + a, 4) == 0 && memcmp(r + 4 + a, r0 + 4 + a, 4) == 0;
    const uint32_t code = !same ? 0u : memcmp(r + flat, r0 + flat, 4) == 0 ? 1u : memcmp(r + flat, r0 + 4 + flat, 4) == 0 ? 2u : 0u;
    memcpy(r + 7, &code, 4);
    s.n_hull += code != 0u;
  }
  // a is an ancestor of k iff a < k < skip(a) (a leaf's skip is a + 1)
  for (size_t k = 0; k < n_kept; ++k) {
    if (tri_of(k) < 0) continue;
    uint64_t need = 1ull << box_id[k];
    for (size_t a = 0; a < k; ++a)
      if (skip_of(a) > k) need |= 1ull << box_id[a];
    s.need.push_back(need);
    s.slot.push_back(tri_of(k));
  }
  s.n_leaves = (int)s.need.size();
  // under[b]: the leaves box b guards, as the bit pattern of the record's
  // fourth word (sweep_walk.h sweep_cands; slab never reads it)
  s.under.assign((size_t)s.n_boxes, 0u);
  for (int l = 0; l < s.n_leaves; ++l)
    for (int b = 0; b < s.n_boxes; ++b)
      if (s.need[(size_t)l] >> b & 1u) s.under[(size_t)b] |= 1u << l;
  for (int b = 0; b < s.n_boxes; ++b) memcpy(&s.boxes[8 * (size_t)b + 3], &s.under[(size_t)b], 4);
  // the cube table: every box past the root has a hull code (so none is general), one box per (axis, code)
  s.cube = true;
  s.cube_all = s.under[0];
  bool taken[6] = {false, false, false, false, false, false};
  for (int b = 1; b < s.n_boxes && s.cube; ++b) {
    const float* r = &s.boxes[8 * (size_t)b];
    uint32_t code;
    memcpy(&code, r + 7, 4);
    int flat = -1;
    for (int a = 2; a >= 0; --a)
      if (memcmp(r + a, r + 4 + a, 4) == 0) flat = a;   // the first flat axis: the one the code is about
    if (flat < 0 || (code != 1u && code != 2u) || taken[2 * flat + (int)code - 1]) {
      s.cube = false;
      break;
    }
    taken[2 * flat + (int)code - 1] = true;
    s.cube_under[2 * flat + (int)code - 1] = s.under[(size_t)b];
  }
  if (!s.cube) s.cube_all = 0u, memset(s.cube_under, 0, sizeof s.cube_under);
  *out = s;
  return true;
}

}  // namespace pt
