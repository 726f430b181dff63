// Test infrastructure: a stand-alone program that runs the host statement of the batched ray queries
// (csrc/pt_rays_host.cpp, what pt_trace_rays_host calls) on generated scenes and rays, for a run under a
// host address / undefined-behaviour sanitizer.  It links the statement, the threaded-tree check it
// validates with and the host BVH builder -- no HIP runtime, no library, nothing from the oracle.
// Built by tests/native.py (tests/test_rays.py); prints one line per scene and "rays_check ok".
//
// What it checks beside memory safety: an independent brute-force closest hit over every triangle
// (pt_isect.h tri_test, least t, ties to the lowest index) agrees with the walk in t wherever no slab test
// can have hidden the winner -- rays with finite 1/d on every axis, where a leaf's box passes whenever its
// triangle is hit up to rounding; those cases are counted, not asserted bit for bit, since a leaf box may
// miss a grazing hit.  The occlusion answer agrees with the closest hit: occluded iff hit and !(t >= limit)
// (the least accepted t decides).  The thread count does not change a word of the output.  Arrays that
// are not a scene are refused.  And plan_rays (pt_device.h), the pure choice of launch_rays' kernels and grids, is
// table-tested here.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "pt_device.h"
#include "pt_isect.h"
#include "pt_rays_host.h"
#include "scene/bvh.h"

using namespace ptd;

namespace {

struct Mesh {
  std::vector<float> v;
  std::vector<uint32_t> idx;
  std::vector<pt::BVHNode> nodes;
};

bool build(const std::vector<float>& v, const std::vector<uint32_t>& i, bool int_bits, Mesh* m) {
  m->v = v;
  m->idx.assign(i.size(), 0);
  m->nodes.assign(2 * (i.size() / 3) - 1, pt::BVHNode{});
  pt::BVHOptions o;
  o.encoding = int_bits ? pt::BVHEncoding::kIntBits : pt::BVHEncoding::kFloat;
  o.threads = 2;
  std::string err;
  if (pt::build_bvh(v.data(), v.size(), i.data(), i.size(), m->idx.data(), m->nodes.data(), o, &err) != 0) {
    fprintf(stderr, "build_bvh: %s\n", err.c_str());
    return false;
  }
  return true;
}

void cloud(int n, uint32_t seed, std::vector<float>* v, std::vector<uint32_t>* i) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<float> c(-1.0f, 1.0f), o(-0.05f, 0.05f);
  for (int t = 0; t < n; ++t) {
    const float cx = c(g), cy = c(g), cz = c(g);
    for (int k = 0; k < 3; ++k) {
      v->push_back(cx + o(g));
      v->push_back(cy + o(g));
      v->push_back(cz + o(g));
      i->push_back((uint32_t)(3 * t + k));
    }
  }
}

// axis-aligned quads sharing edges: equal-t ties
void grid(int n, std::vector<float>* v, std::vector<uint32_t>* i) {
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      const uint32_t base = (uint32_t)(v->size() / 3);
      const float x0 = -1.0f + 2.0f * (float)a / (float)n, y0 = -1.0f + 2.0f * (float)b / (float)n, s = 2.0f / (float)n;
      const float q[4][3] = {{x0, y0, 0.0f}, {x0 + s, y0, 0.0f}, {x0 + s, y0 + s, 0.0f}, {x0, y0 + s, 0.0f}};
      for (auto& p : q) v->insert(v->end(), p, p + 3);
      const uint32_t t[6] = {base, base + 1, base + 2, base, base + 2, base + 3};
      i->insert(i->end(), t, t + 6);
    }
}

std::vector<float> rays_for(size_t n, uint32_t seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<float> u(-1.5f, 1.5f), l(0.0f, 4.0f);
  std::normal_distribution<float> nd;
  std::vector<float> r(8 * n, 0.0f);
  const float odd[] = {0.0f, -0.0f, 1e-45f, -1e-41f, INFINITY, -INFINITY, NAN, 1e20f, 1e-3f, 1e3f};
  for (size_t k = 0; k < n; ++k) {
    float* p = &r[8 * k];
    float d[3] = {nd(g), nd(g), nd(g)};
    const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int a = 0; a < 3; ++a) {
      p[a] = u(g);
      p[3 + a] = d[a] / len;
    }
    p[6] = l(g);
    if (k % 5 == 1) p[3 + k % 3] = 0.0f;                    // a zero direction component
    if (k % 5 == 2) p[k % 3] = (k & 8) ? 1.0f : -1.0f;      // the origin on a coordinate the grid uses
    if (k % 11 == 3) p[(k / 11) % 7] = odd[(k / 77) % 10];  // hostile words, origin, direction or limit
    if (k % 13 == 4) p[6] = odd[(k / 13) % 10];
    if (k % 17 == 5) {                                      // straight down at the grid's vertices and edges
      p[0] = -1.0f + 0.25f * (float)(k % 9);
      p[1] = -1.0f + 0.25f * (float)((k / 9) % 9);
      p[2] = 1.0f;
      p[3] = p[4] = 0.0f;
      p[5] = -1.0f;
    }
  }
  return r;
}

int check_scene(const char* name, const Mesh& m, bool int_bits, size_t n_rays, uint32_t seed) {
  const std::vector<float> rays = rays_for(n_rays, seed);
  std::vector<float> hits(8 * n_rays, -7.0f), hits1(8 * n_rays, -9.0f);
  std::vector<uint32_t> occ(n_rays, 7u), occ1(n_rays, 9u);
  const float* nodes = (const float*)m.nodes.data();
  std::string why = ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), nodes, m.nodes.size(),
                                         int_bits, 0, rays.data(), n_rays, hits.data(), 3);
  if (why.empty())
    why = ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), nodes, m.nodes.size(), int_bits, 0,
                               rays.data(), n_rays, hits1.data(), 1);
  if (why.empty())
    why = ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), nodes, m.nodes.size(), int_bits, 1,
                               rays.data(), n_rays, occ.data(), 4);
  if (why.empty())
    why = ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), nodes, m.nodes.size(), int_bits, 1,
                               rays.data(), n_rays, occ1.data(), 1);
  if (!why.empty()) {
    fprintf(stderr, "%s: refused: %s\n", name, why.c_str());
    return 1;
  }
  if (memcmp(hits.data(), hits1.data(), hits.size() * 4) != 0 || occ != occ1) {
    fprintf(stderr, "%s: the thread count changed the output\n", name);
    return 1;
  }
  const size_t nt = m.idx.size() / 3;
  size_t n_hit = 0, n_occ = 0, brute_same = 0, brute_checked = 0;
  for (size_t k = 0; k < n_rays; ++k) {
    const float* r = &rays[8 * k];
    const float* h = &hits[8 * k];
    int32_t tri;
    memcpy(&tri, &h[1], 4);
    const bool hit = tri >= 0;
    if (tri < -1 || (size_t)(tri + 1) > nt || f2u(h[7]) != 0u) {
      fprintf(stderr, "%s: ray %zu: bad record (tri %d)\n", name, k, tri);
      return 1;
    }
    if (!hit && (f2u(h[0]) != f2u(1e30f) || f2u(h[2]) | f2u(h[3]) | f2u(h[4]) | f2u(h[5]) | f2u(h[6]))) {
      fprintf(stderr, "%s: ray %zu: a miss is {1e30, -1, 0...}\n", name, k);
      return 1;
    }
    if (hit && !(h[0] > 1e-6f && h[0] < 1e30f && h[2] >= 0.0f && h[3] >= 0.0f && h[2] + h[3] <= 1.0f)) {
      fprintf(stderr, "%s: ray %zu: t %g u %g v %g outside intersectTriangle's accept\n", name, k, h[0], h[2], h[3]);
      return 1;
    }
    const bool want_occ = hit && !(h[0] >= r[6]);
    if ((occ[k] != 0u) != want_occ || occ[k] > 1u) {
      fprintf(stderr, "%s: ray %zu: occlusion %u, closest t %g, limit %g\n", name, k, occ[k], h[0], r[6]);
      return 1;
    }
    n_hit += hit;
    n_occ += occ[k];
    const v3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    if (!(fabsf(1.0f / d.x) < 1e30f && fabsf(1.0f / d.y) < 1e30f && fabsf(1.0f / d.z) < 1e30f)) continue;
    float best = 1e30f;
    for (size_t t = 0; t < nt; ++t) {
      v3 p[3];
      for (int c = 0; c < 3; ++c) {
        const float* v = &m.v[3 * (size_t)m.idx[3 * t + c]];
        p[c] = mk(v[0], v[1], v[2]);
      }
      const v3 e1 = sub(p[1], p[0]), e2 = sub(p[2], p[0]);
      float tt;
      if (tri_test(o, d, make_float4(p[0].x, p[0].y, p[0].z, e1.x), make_float4(e1.y, e1.z, e2.x, e2.y),
                   make_float4(e2.z, 0.0f, 0.0f, 0.0f), &tt) && tt < best)
        best = tt;
    }
    ++brute_checked;
    brute_same += f2u(best) == f2u(h[0]);
    if (best > h[0]) {   // the walk tests a subset of the triangles: it cannot find a nearer hit
      fprintf(stderr, "%s: ray %zu: walk t %g below every triangle's (%g)\n", name, k, h[0], best);
      return 1;
    }
  }
  printf("%s: %zu rays, %zu hits, %zu occluded, brute force agrees on %zu of %zu\n", name, n_rays, n_hit, n_occ,
         brute_same, brute_checked);
  if (n_hit == 0 || n_hit == n_rays || brute_same * 100 < brute_checked * 99) {
    fprintf(stderr, "%s: the rays do not exercise the walk\n", name);
    return 1;
  }
  return 0;
}

int check_refusals(const Mesh& m) {
  std::vector<float> rays = rays_for(4, 1), hits(32);
  const float* nodes = (const float*)m.nodes.data();
  std::vector<uint32_t> bad_idx = m.idx;
  bad_idx[1] = (uint32_t)(m.v.size() / 3);
  std::vector<pt::BVHNode> loop = m.nodes;
  loop[0].minBounds[3] = 0.0f;   // the root its own child
  std::vector<pt::BVHNode> far = m.nodes;
  far[0].maxBounds[3] = (float)(m.nodes.size() + 5);
  int bad = 0;
  bad += ptr::trace_rays_host(m.v.data(), m.v.size(), bad_idx.data(), bad_idx.size(), nodes, m.nodes.size(), false, 0,
                              rays.data(), 4, hits.data(), 1).empty();
  bad += ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), (const float*)loop.data(), loop.size(),
                              false, 0, rays.data(), 4, hits.data(), 1).empty();
  bad += ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), (const float*)far.data(), far.size(),
                              false, 0, rays.data(), 4, hits.data(), 1).empty();
  bad += ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size() - 3, nodes, m.nodes.size(), false, 0,
                              rays.data(), 4, hits.data(), 1).empty();
  bad += ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), 0, nodes, 0, false, 0, rays.data(), 4, hits.data(), 1)
             .empty();
  // no rays: nothing is read or written
  bad += !ptr::trace_rays_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), nodes, m.nodes.size(), false, 1, nullptr,
                               0, nullptr, 4).empty();
  if (bad) fprintf(stderr, "refusals: %d wrong\n", bad);
  return bad;
}

// plan_rays (pt_device.h), the pure choice of launch_rays' kernels, grids and LDS bytes.
int check_plan() {
  int bad = 0;
  auto expect = [&bad](bool ok, const char* what) {
    if (!ok) {
      fprintf(stderr, "plan_rays: %s\n", what);
      ++bad;
    }
  };
  RenderParams p{};
  p.n_nodes = 23;
  p.n_tris = 12;
  p.wf_grid = 100;
  expect(plan_rays(p, 0, 0, false, true, 0).what == Launch::Nothing, "no rays: nothing");
  expect(plan_rays(p, 2, 10, false, true, 0).what == Launch::Refused, "an unknown kind");
  expect(plan_rays(p, 1, kRaysMax + 1, false, true, 0).what == Launch::Refused, "too many rays");
  expect(plan_rays(p, 1, -1, false, true, 0).what == Launch::Refused, "a negative count");
  RaysLaunch l = plan_rays(p, 1, kRaysMax, false, true, 0);
  expect(l.what == Launch::Run && !l.wide && l.exact_v == RaysExactVariant{1, false} && l.grid_exact == (kRaysMax + 255) / 256 &&
             l.grid_exact <= 0x7fffffffll && l.lds == 0, "the exact kernel from device memory, a workgroup per 256 rays");
  l = plan_rays(p, 0, 1000, true, false, 0);
  expect(l.what == Launch::Run && l.exact_v == RaysExactVariant{0, true} && l.grid_exact == 4 && l.lds == scene_lds_bytes(p),
         "the exact kernel from LDS");
  l = plan_rays(p, 0, 10000000, true, false, 0);
  expect(l.what == Launch::Run && l.grid_exact == kRaysLdsGrid, "the LDS-staged grid is bounded");
  p.n_tris = 2000;
  p.n_nodes = 3999;
  expect(plan_rays(p, 0, 1000, true, false, 0).what == Launch::Refused, "a scene too large for LDS");
  expect(plan_rays(p, 0, 1000, false, false, 0).what == Launch::Run, "... walks from device memory");
  const float4 dummy = make_float4(0, 0, 0, 0);
  p.wide = &dummy;
  p.wide_qn = 1;
  p.wide_ovf_lanes = 256 * 100;
  l = plan_rays(p, 1, 1 << 20, true, true, 1536);
  expect(l.what == Launch::Run && l.wide && l.wide_v == RaysWideVariant{1, true, true} && l.grid_wide == 100 &&
             l.exact_v == RaysExactVariant{1, false} && l.grid_exact == 4096 && l.lds == 0,
         "the wide kernel's grid is bounded by the overflow areas; the marked launch reads device memory");
  p.wide_ovf_lanes = 256 * 4000;
  l = plan_rays(p, 0, 1 << 20, false, false, 1536);
  expect(l.grid_wide == 1536 && l.wide_v == RaysWideVariant{0, true, false}, "... by the resident workgroups");
  l = plan_rays(p, 0, 1000, false, false, 1536);
  expect(l.grid_wide == 4, "... by the batch");
  p.wf_grid = 1;
  expect(plan_rays(p, 0, 1 << 20, false, true, 1536).grid_wide == 15, "PT_OPT_WF_GRID 1: a hundredth of the grid");
  expect(plan_rays(p, 0, 1 << 20, false, true, 40).grid_wide == 1, "... and at least one workgroup");
  p.wide_qn = 0;
  expect(plan_rays(p, 0, 100, false, true, 40).wide_v == RaysWideVariant{0, false, true}, "the 128-B layout");
  p.wide_ovf_lanes = 255;
  expect(plan_rays(p, 0, 100, false, true, 40).what == Launch::Refused, "no overflow areas");
  p.wide_ovf_lanes = 256;
  expect(plan_rays(p, 0, 100, false, true, 0).what == Launch::Refused, "no resident workgroup");
  return bad;
}

}  // namespace

int main() {
  int bad = check_plan();
  {
    std::vector<float> v;
    std::vector<uint32_t> i;
    cloud(600, 11, &v, &i);
    Mesh m;
    if (!build(v, i, false, &m)) return 1;
    bad += check_scene("cloud600", m, false, 4000, 1);
    bad += check_refusals(m);
    Mesh mi;
    if (!build(v, i, true, &mi)) return 1;
    bad += check_scene("cloud600/int-bits", mi, true, 1500, 2);
  }
  {
    std::vector<float> v;
    std::vector<uint32_t> i;
    grid(8, &v, &i);
    Mesh m;
    if (!build(v, i, false, &m)) return 1;
    bad += check_scene("grid8", m, false, 4000, 3);
  }
  {   // one triangle: a tree of one node
    const std::vector<float> v = {-1.0f, -1.0f, 0.0f, 1.0f, -1.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    const std::vector<uint32_t> i = {0, 1, 2};
    Mesh m;
    if (!build(v, i, false, &m)) return 1;
    bad += check_scene("one", m, false, 1000, 4);
  }
  if (bad) return 1;
  printf("rays_check ok\n");
  return 0;
}
