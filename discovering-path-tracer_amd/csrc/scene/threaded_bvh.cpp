#include "threaded_bvh.h"

#include <math.h>
#include <string.h>

namespace pt {

std::string thread_bvh(const float* nodes, size_t n, bool int_bits, size_t n_tris, std::vector<float>* out) {
  if (n == 0 || n > 0x7fffffffull) return "BVH has no nodes or too many";
  std::vector<int32_t> left(n), right(n);
  for (size_t i = 0; i < n; ++i) {
    float lw = nodes[8 * i + 3], rw = nodes[8 * i + 7];
    int32_t l, r;
    if (int_bits) {
      memcpy(&l, &lw, 4);
      memcpy(&r, &rw, 4);
    } else {
      // int(node.minBounds.w) (raytrace_comp.comp:173-174): only exact
      // below 2^24, so refuse anything the float cannot hold exactly.
      if (!(lw == floorf(lw)) || !(rw == floorf(rw)) || fabsf(lw) >= 16777216.0f || fabsf(rw) >= 16777216.0f)
        return "float-encoded BVH index is not an exact integer below 2^24 (node " + std::to_string(i) +
               "); rebuild with PT_NODES_INT_BITS";
      l = (int32_t)lw;
      r = (int32_t)rw;
    }
    left[i] = l;
    right[i] = r;
    if (l == -1) {
      if (r < 0 || (size_t)r >= n_tris) return "leaf " + std::to_string(i) + " has triangle index out of range";
    } else if (l < 0 || (size_t)l >= n || r < 0 || (size_t)r >= n) {
      return "node " + std::to_string(i) + " has child index out of range";
    }
  }
  std::vector<int32_t> order;
  order.reserve(n);
  std::vector<int32_t> newidx(n, -1);
  std::vector<int32_t> stack;
  stack.push_back(0);
  while (!stack.empty()) {
    const int32_t v = stack.back();
    stack.pop_back();
    if (newidx[v] != -1) return "BVH node reachable twice (not a tree)";
    newidx[v] = (int32_t)order.size();
    order.push_back(v);
    if (left[v] != -1) {
      stack.push_back(left[v]);    // :198  push left
      stack.push_back(right[v]);   // :199  push right -> popped first
    }
  }
  const size_t m = order.size();
  std::vector<int32_t> size(n, 1);
  for (size_t k = m; k-- > 0;) {
    const int32_t v = order[k];
    if (left[v] != -1) size[v] = 1 + size[left[v]] + size[right[v]];
  }
  // A child whose bounds are bitwise its parent's is hit whenever it is
  // visited (it is only visited after its parent was hit by the same ray, and
  // the slab test is a pure function of ray and bounds): flag it in bit 31 of
  // `skip` so the kernel can skip recomputing the test.
  std::vector<int32_t> parent(n, -1);
  for (size_t k = 0; k < m; ++k) {
    const int32_t v = order[k];
    if (left[v] != -1) parent[left[v]] = parent[right[v]] = v;
  }
  auto same_bounds = [&](int32_t a, int32_t b) {
    return memcmp(nodes + 8 * (size_t)a, nodes + 8 * (size_t)b, 12) == 0 &&
           memcmp(nodes + 8 * (size_t)a + 4, nodes + 8 * (size_t)b + 4, 12) == 0;
  };
  out->assign(8 * m, 0.0f);
  for (size_t k = 0; k < m; ++k) {
    const int32_t v = order[k];
    const float* nd = nodes + 8 * (size_t)v;
    const bool implied = parent[v] >= 0 && same_bounds(v, parent[v]);
    const int32_t skip = (int32_t)(((uint32_t)k + (uint32_t)size[v]) | (implied ? 0x80000000u : 0u));
    const int32_t tri = left[v] == -1 ? right[v] : -1;
    float* o = out->data() + 8 * k;
    memcpy(o, nd, 12);
    memcpy(o + 3, &skip, 4);
    memcpy(o + 4, nd + 4, 12);
    memcpy(o + 7, &tri, 4);
  }
  return "";
}

void collapse_implied(const std::vector<float>& full, std::vector<float>* out) {
  const size_t m = full.size() / 8;
  auto raw_skip = [&](size_t k) { int32_t s; memcpy(&s, &full[8 * k + 3], 4); return s; };
  auto tri_of = [&](size_t k) { int32_t t; memcpy(&t, &full[8 * k + 7], 4); return t; };
  auto dropped = [&](size_t k) { return raw_skip(k) < 0 && tri_of(k) < 0; };
  std::vector<int32_t> nxt(m + 1);
  int32_t kept = 0;
  for (size_t k = 0; k < m; ++k)
    if (!dropped(k)) ++kept;
  nxt[m] = kept;
  for (size_t k = m; k-- > 0;) nxt[k] = dropped(k) ? nxt[k + 1] : --kept;
  out->clear();
  out->reserve(8 * (size_t)nxt[m]);
  for (size_t k = 0; k < m; ++k) {
    if (dropped(k)) continue;
    const int32_t raw = raw_skip(k);
    const int32_t skip = (int32_t)((uint32_t)nxt[raw & 0x7fffffff] | ((uint32_t)raw & 0x80000000u));
    out->insert(out->end(), full.begin() + 8 * k, full.begin() + 8 * k + 8);
    memcpy(&(*out)[out->size() - 5], &skip, 4);
  }
}

}  // namespace pt
