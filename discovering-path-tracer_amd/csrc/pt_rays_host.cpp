// pt_rays_host.cpp — pt_trace_rays_host's walk (pt_rays_host.h).
#include "pt_rays_host.h"

#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "pt_isect.h"
#include "scene/threaded_bvh.h"

namespace ptr {
using namespace ptd;

// traceRay: the explicit stack, left pushed first and right popped first (:198-199), strict '<' (:185).
// limit null: the closest hit; else the occlusion query, which may stop at the first triangle that settles it.
bool walk(const Scene& s, v3 o, v3 d, const float* limit, std::vector<int32_t>& stack, float* best, int32_t* bt) {
  const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
  *best = 1e30f;
  *bt = -1;
  stack.clear();
  stack.push_back(0);
  while (!stack.empty()) {
    const int32_t k = stack.back();
    stack.pop_back();
    const float* nd = s.nodes + 8 * (size_t)k;
    if (!slab(o, inv, make_float4(nd[0], nd[1], nd[2], 0.0f), make_float4(nd[4], nd[5], nd[6], 0.0f))) continue;
    if (s.left[(size_t)k] == -1) {
      const int32_t tri = s.right[(size_t)k];
      const float4* T = s.tris.data() + 3 * (size_t)tri;
      float t;
      if (!tri_test(o, d, T[0], T[1], T[2], &t)) continue;
      if (limit) {
        if (t < 1e30f && !(t >= *limit)) return true;
      } else if (t < *best) {
        *best = t;
        *bt = tri;
      }
    } else {
      stack.push_back(s.left[(size_t)k]);
      stack.push_back(s.right[(size_t)k]);
    }
  }
  return false;
}

namespace {

void run(const Scene& s, int kind, const float* rays, size_t i0, size_t i1, void* out) {
  std::vector<int32_t> stack;
  stack.reserve(64);
  for (size_t i = i0; i < i1; ++i) {
    const float* r = rays + 8 * i;
    const v3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    float t;
    int32_t tri;
    if (kind == 1) {
      ((uint32_t*)out)[i] = walk(s, o, d, &r[6], stack, &t, &tri) ? 1u : 0u;
      continue;
    }
    (void)walk(s, o, d, nullptr, stack, &t, &tri);
    float h[8] = {1e30f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (tri >= 0) {
      const float4* T = s.tris.data() + 3 * (size_t)tri;
      h[0] = t;
      tri_uv(o, d, T[0], T[1], T[2], &h[2], &h[3]);
      h[4] = T[2].y;
      h[5] = T[2].z;
      h[6] = T[2].w;
    }
    memcpy(&h[1], &tri, 4);
    memcpy((float*)out + 8 * i, h, sizeof h);
  }
}

}  // namespace

std::string make_scene(const float* V, size_t nvf, const uint32_t* I, size_t ni, const float* nodes, size_t nn,
                       bool int_bits, Scene* out) {
  Scene& s = *out;
  if (nvf % 3 || ni % 3 || ni == 0) return "vertex/index array sizes must be non-zero multiples of 3";
  const size_t nt = ni / 3, nv = nvf / 3;
  if (nn != 2 * nt - 1) return "expected 2T-1 = " + std::to_string(2 * nt - 1) + " nodes, got " + std::to_string(nn);
  if (nt > 0x7fffffffull) return "too many triangles";
  for (size_t i = 0; i < ni; ++i)
    if (I[i] >= nv) return "vertex index out of range at " + std::to_string(i);
  s.nodes = nodes;
  {   // a tree of valid links (the walk then ends, and reads inside the arrays)
    std::vector<float> threaded;
    const std::string why = pt::thread_bvh(nodes, nn, int_bits, nt, &threaded);
    if (!why.empty()) return why;
  }
  s.left.resize(nn);
  s.right.resize(nn);
  for (size_t k = 0; k < nn; ++k) {
    const float lw = nodes[8 * k + 3], rw = nodes[8 * k + 7];
    if (int_bits) {
      memcpy(&s.left[k], &lw, 4);
      memcpy(&s.right[k], &rw, 4);
    } else {   // int(node.minBounds.w) (:173-174); thread_bvh has checked the floats are exact integers
      s.left[k] = (int32_t)lw;
      s.right[k] = (int32_t)rw;
    }
  }
  s.tris.resize(3 * nt);
  for (size_t t = 0; t < nt; ++t) {   // the ops of setup_tris_kernel
    v3 p[3];
    for (int c = 0; c < 3; ++c) {
      const float* v = V + 3 * (size_t)I[3 * t + c];
      p[c] = mk(v[0], v[1], v[2]);
    }
    const v3 e1 = sub(p[1], p[0]), e2 = sub(p[2], p[0]);
    const v3 nr = normalize(cross(e1, e2));
    s.tris[3 * t] = make_float4(p[0].x, p[0].y, p[0].z, e1.x);
    s.tris[3 * t + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
    s.tris[3 * t + 2] = make_float4(e2.z, nr.x, nr.y, nr.z);
  }
  return "";
}

std::string trace_rays_host(const float* V, size_t nvf, const uint32_t* I, size_t ni, const float* nodes, size_t nn,
                            bool int_bits, int kind, const float* rays, size_t n, void* out, int threads) {
  Scene s;
  const std::string bad = make_scene(V, nvf, I, ni, nodes, nn, int_bits, &s);
  if (!bad.empty()) return bad;
  size_t nth = threads > 0 ? (size_t)threads : std::max(1u, std::thread::hardware_concurrency());
  nth = std::min<size_t>(std::min<size_t>(nth, 256), std::max<size_t>(1, n / 64));
  if (nth <= 1) {
    run(s, kind, rays, 0, n, out);
    return "";
  }
  std::vector<std::thread> pool;
  const size_t per = (n + nth - 1) / nth;
  for (size_t k = 0; k < nth; ++k) {
    const size_t i0 = std::min(n, k * per), i1 = std::min(n, i0 + per);
    if (i0 < i1) pool.emplace_back([&s, kind, rays, i0, i1, out] { run(s, kind, rays, i0, i1, out); });
  }
  for (auto& th : pool) th.join();
  return "";
}

}  // namespace ptr
