// Test infrastructure: a stand-alone program that runs the host statement of the radiance queries
// (csrc/pt_radiance_host.cpp, what pt_trace_radiance_host and pt_camera_rays_host call) on generated scenes,
// lights and rays, for a run under a host address / undefined-behaviour sanitizer.  It links the statement, the
// ray walk it shares with the ray queries, the threaded-tree check and the host BVH builder -- no HIP runtime, no
// library, nothing from the oracle.  Built by tests/native.py (tests/test_radiance.py); prints one line per
// check and "radiance_check ok".
//
// What it checks beside memory safety: the thread count does not change a byte; S samples equal the running
// mean of S single-sample queries at the strided seeds, the uint32 wrap included; alpha is 1; a ray that
// looks into an unoccluded light returns its intensity; no light and max_depth 0 give +0; rays with NaN,
// infinite, zero and subnormal components return; camera rays carry their seed and a pixel list equals the
// raster order; arrays that are not a scene are refused.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "pt_radiance_host.h"
#include "scene/bvh.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                   \
  do {                                                 \
    if (!(cond)) {                                     \
      printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++failures;                                      \
    }                                                  \
  } while (0)

struct Mesh {
  std::vector<float> v;
  std::vector<uint32_t> idx;
  std::vector<pt::BVHNode> nodes;
};

bool build(const std::vector<float>& v, const std::vector<uint32_t>& i, Mesh* m) {
  m->v = v;
  m->idx.assign(i.size(), 0);
  m->nodes.assign(2 * (i.size() / 3) - 1, pt::BVHNode{});
  pt::BVHOptions o;
  o.threads = 2;
  std::string err;
  if (pt::build_bvh(v.data(), v.size(), i.data(), i.size(), m->idx.data(), m->nodes.data(), o, &err) != 0) {
    fprintf(stderr, "build_bvh: %s\n", err.c_str());
    return false;
  }
  return true;
}

// a floor quad at y = 0 and a cloud of small triangles above it
void scene(int n, uint32_t seed, std::vector<float>* v, std::vector<uint32_t>* i) {
  const float q[4][3] = {{-2, 0, -2}, {2, 0, -2}, {2, 0, 2}, {-2, 0, 2}};
  for (auto& p : q) v->insert(v->end(), p, p + 3);
  const uint32_t t[6] = {0, 2, 1, 0, 3, 2};
  i->insert(i->end(), t, t + 6);
  std::mt19937 g(seed);
  std::uniform_real_distribution<float> c(-1.0f, 1.0f), h(0.2f, 1.2f), o(-0.15f, 0.15f);
  for (int k = 0; k < n; ++k) {
    const float cx = c(g), cy = h(g), cz = c(g);
    const uint32_t base = (uint32_t)(v->size() / 3);
    for (int a = 0; a < 3; ++a) {
      v->push_back(cx + o(g));
      v->push_back(cy + o(g));
      v->push_back(cz + o(g));
      i->push_back(base + (uint32_t)a);
    }
  }
}

std::vector<float> queries(size_t n, uint32_t seed, bool hostile) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<float> u(-1.5f, 1.5f);
  std::normal_distribution<float> nd;
  const float odd[] = {0.0f, -0.0f, 1e-45f, -1e-41f, INFINITY, -INFINITY, NAN, 1e20f, 1e-3f, 1e3f};
  std::vector<float> r(8 * n, 0.0f);
  for (size_t k = 0; k < n; ++k) {
    float* p = &r[8 * k];
    float d[3] = {nd(g), -fabsf(nd(g)) - 0.2f, nd(g)};
    const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    p[0] = u(g);
    p[1] = 2.5f;
    p[2] = u(g);
    for (int a = 0; a < 3; ++a) p[3 + a] = d[a] / len;
    if (hostile) p[(k / 10) % 6] = odd[k % 10];
    p[6] = 1e30f;
    const uint32_t s = (uint32_t)(k * 2654435761u + seed);
    memcpy(&p[7], &s, 4);
  }
  return r;
}

std::string trace(const Mesh& m, const std::vector<float>& lights, int depth, int sss, uint32_t S, uint32_t stride,
                  const std::vector<float>& rays, std::vector<float>* out, int threads) {
  out->assign(rays.size() / 2, -1.0f);
  return ptr::trace_radiance_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size(), (const float*)m.nodes.data(),
                                  m.nodes.size(), false, lights.data(), lights.size() / 16, depth, sss, S, stride,
                                  rays.data(), rays.size() / 8, out->data(), threads);
}

}  // namespace

int main() {
  std::vector<float> v;
  std::vector<uint32_t> idx;
  scene(60, 7, &v, &idx);
  Mesh m;
  if (!build(v, idx, &m)) return 1;
  // position, normal, intensity, size (pt_area_light): one above the scene looking down, one to the side
  const std::vector<float> one = {0, 3, 0, 0, 0, -1, 0, 0, 10, 10, 10, 0, 2.5f, 2.5f, 0, 0};
  std::vector<float> two = one;
  const float second[16] = {3, 1, 0, 0, -1, 0, 0, 0, 2, 4, 8, 0, 1, 1, 0, 0};
  two.insert(two.end(), second, second + 16);
  const std::vector<float> none;
  const std::vector<float> rays = queries(600, 11, false);
  std::vector<float> a, b, c;

  // thread counts
  EXPECT(trace(m, two, 4, 3, 1, 1, rays, &a, 1).empty());
  EXPECT(trace(m, two, 4, 3, 1, 1, rays, &b, 3).empty());
  EXPECT(trace(m, two, 4, 3, 1, 1, rays, &c, 16).empty());
  EXPECT(!memcmp(a.data(), b.data(), a.size() * 4) && !memcmp(a.data(), c.data(), a.size() * 4));
  size_t lit = 0, black = 0;
  for (size_t k = 0; k < rays.size() / 8; ++k) {
    EXPECT(a[4 * k + 3] == 1.0f);
    const bool z = a[4 * k] == 0.0f && a[4 * k + 1] == 0.0f && a[4 * k + 2] == 0.0f;
    lit += !z;
    black += z;
  }
  EXPECT(lit >= 100);
  printf("threads ok: %zu lit, %zu black of %zu\n", lit, black, rays.size() / 8);

  // S samples = the fold of S single-sample queries, with the wrap
  const uint32_t strides[] = {1u, 384u, 0xFFFFFFFFu};
  const uint32_t counts[] = {2u, 5u, 64u};
  const std::vector<float> few(rays.begin(), rays.begin() + 8 * 40);
  for (uint32_t stride : strides)
    for (uint32_t S : counts) {
      EXPECT(trace(m, two, 2, 1, S, stride, few, &a, 2).empty());
      std::vector<float> acc(few.size() / 2, 0.0f);
      for (uint32_t s = 0; s < S; ++s) {
        std::vector<float> q = few;
        for (size_t k = 0; k < q.size() / 8; ++k) {
          uint32_t seed;
          memcpy(&seed, &q[8 * k + 7], 4);
          seed += s * stride;
          memcpy(&q[8 * k + 7], &seed, 4);
        }
        EXPECT(trace(m, two, 2, 1, 1, 1, q, &b, 1).empty());
        const float fb = (float)s, fb1 = (float)(s + 1u);
        for (size_t k = 0; k < q.size() / 8; ++k) {
          // a single-sample answer is (0 * 0 + c) / 1: c but for the sign of zero, and the fold adds to it
          for (int ch = 0; ch < 3; ++ch) acc[4 * k + ch] = (acc[4 * k + ch] * fb + b[4 * k + ch]) / fb1;
          acc[4 * k + 3] = (acc[4 * k + 3] * fb + 1.0f) / fb1;
        }
      }
      EXPECT(!memcmp(a.data(), acc.data(), a.size() * 4));
      printf("S=%u stride=%u ok\n", S, stride);
    }

  // looking up into the first light from below it, nothing between: its intensity; no light, depth 0: +0
  {
    std::vector<float> up = {0.0f, 2.0f, 0.0f, 0.0f, 1.0f, 0.0f, 1e30f, 0.0f};
    EXPECT(trace(m, one, 4, 3, 1, 1, up, &a, 1).empty());
    EXPECT(a[0] == 10.0f && a[1] == 10.0f && a[2] == 10.0f && a[3] == 1.0f);
    EXPECT(trace(m, none, 0, 3, 4, 1, rays, &a, 2).empty());
    bool zero = true;
    for (size_t k = 0; k < a.size(); ++k) {
      uint32_t w;
      memcpy(&w, &a[k], 4);
      zero = zero && (k % 4 == 3 ? a[k] == 1.0f : w == 0u);
    }
    EXPECT(zero);
    EXPECT(trace(m, none, 4, 3, 1, 1, rays, &a, 2).empty());
    printf("light and no-light ok\n");
  }

  // hostile rays return, and repeat across thread counts (NaN payloads included: the same code ran)
  {
    const std::vector<float> bad = queries(600, 13, true);
    EXPECT(trace(m, two, 4, 3, 2, 7, bad, &a, 1).empty());
    EXPECT(trace(m, two, 4, 3, 2, 7, bad, &b, 5).empty());
    EXPECT(!memcmp(a.data(), b.data(), a.size() * 4));
    printf("hostile ok\n");
  }

  // camera rays
  {
    const float cam[16] = {0, 1, 4, 0, 0, -0.1f, -1, 0, 0, 1, 0, 0, 45, 0, 0, 0};
    const int W = 24, H = 16;
    std::vector<float> all(8 * W * H), some(8 * 5);
    ptr::camera_rays_host(cam, W, H, 3, nullptr, (size_t)W * H, all.data());
    const int32_t px[5] = {383, 0, 25, 24, 200};
    ptr::camera_rays_host(cam, W, H, 3, px, 5, some.data());
    for (int k = 0; k < 5; ++k) EXPECT(!memcmp(&some[8 * k], &all[8 * px[k]], 32));
    for (int p = 0; p < W * H; ++p) {
      uint32_t seed;
      memcpy(&seed, &all[8 * p + 7], 4);
      EXPECT(seed == (3u * H + (uint32_t)(p / W)) * W + (uint32_t)(p % W));
      EXPECT(all[8 * p + 6] == 1e30f);
    }
    printf("camera rays ok\n");
  }

  // not a scene
  {
    std::vector<float> out(4);
    const std::vector<float> r = queries(1, 1, false);
    EXPECT(!ptr::trace_radiance_host(m.v.data(), m.v.size(), m.idx.data(), m.idx.size() - 3, (const float*)m.nodes.data(),
                                     m.nodes.size(), false, nullptr, 0, 4, 3, 1, 1, r.data(), 1, out.data(), 1)
                .empty());
  }
  if (failures) {
    printf("radiance_check: %d failures\n", failures);
    return 1;
  }
  printf("radiance_check ok\n");
  return 0;
}
