// Test infrastructure: a stand-alone host program around pt_reproject_host and
// pt_denoise_var_plane_host (csrc/pt_denoise.h, compiled for the host), on the
// shapes the tests use -- for sanitizer runs on the CPU:
//
//   S="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
//      -fno-fast-math -D__HIP_PLATFORM_AMD__ -Iinclude -Idiscovering-path-tracer_amd/csrc"
//   for f in tests/temporal_check.cpp discovering-path-tracer_amd/csrc/*.cpp \
//            discovering-path-tracer_amd/csrc/scene/*.cpp; do
//     hipcc $S -c $f -o san/$(basename $f .cpp).o; done          # host objects, instrumented
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined san/*.o \
//     discovering-path-tracer_amd/build/pt_device.o discovering-path-tracer_amd/build/pt_denoise.o \
//     -lpthread -o temporal_check && ./temporal_check
//
// (the host code under test carries the instrumentation; the program calls
// nothing that touches a GPU, and it is run on the CPU only).
// tests/test_temporal.py builds it plainly against libptamd.so and runs it.
// At 16x16, 37x23 and 64x48 it reprojects seeded images -- guides on the plane
// z = 0 with a block of misses, a depth step and a second normal region in the
// history guide, zero and over-long history lengths, fireflies -- through four
// previous cameras (identical, a 2 degree orbit, looking away, a 60 degree
// orbit) and with no history, filters the result from its variance plane, and
// checks that everything is finite, that lengths stay within n .. max_history
// + n, that alpha passes through and that bad arguments are refused.  Exit
// status 0 and one "ok" line, or 1 and what failed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pathtracer.h"
#include "pt_denoise.h"

namespace {

uint32_t g_state = 2463534242u;
float rnd() {   // xorshift32 -> [0, 1)
  g_state ^= g_state << 13;
  g_state ^= g_state >> 17;
  g_state ^= g_state << 5;
  return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", what);
    ++fails;
  }
}

void camera_at(float x, float y, float z, float dx, float dy, float dz, float cam[16]) {
  memset(cam, 0, 16 * sizeof(float));
  cam[0] = x, cam[1] = y, cam[2] = z;
  cam[4] = dx, cam[5] = dy, cam[6] = dz;
  cam[9] = 1.0f;
  cam[12] = 60.0f;
}

// The camera at distance 5 from the origin, rotated by `deg` about +y, looking at the origin.
void orbit(double deg, float cam[16]) {
  const double a = deg * 3.14159265358979323846 / 180.0;
  camera_at((float)(5.0 * sin(a)), 0.0f, (float)(5.0 * cos(a)), (float)-sin(a), 0.0f, (float)-cos(a), cam);
}

// {n.xyz, t} of cam's guide rays on the plane z = 0.
void plane_guide(const float cam[16], int W, int H, std::vector<float>* g) {
  g->assign((size_t)W * H * 4, 0.0f);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      float o[3], d[3];
      pt_guide_ray(cam, W, H, x, y, o, d);
      float* p = &(*g)[4 * ((size_t)y * W + x)];
      const float t = -o[2] / d[2];
      if (isfinite(t) && t > 0.0f && t < 1e6f)
        p[2] = 1.0f, p[3] = t;
      else
        p[3] = 1e30f;
    }
}

void colours(int W, int H, std::vector<float>* rgba, std::vector<float>* mom) {
  const size_t n = (size_t)W * H;
  rgba->assign(n * 4, 0.0f);
  mom->assign(n * 2, 0.0f);
  for (size_t i = 0; i < n; ++i) {
    float* c = &(*rgba)[4 * i];
    const bool fire = rnd() < 0.05f;
    for (int k = 0; k < 3; ++k) c[k] = 2.0f * rnd() * (fire ? 40.0f : 1.0f);
    c[3] = 0.5f + 0.5f * rnd();
    const float m1 = ptdn::lum(c[0], c[1], c[2]);
    const float spread = (0.05f + 1.45f * rnd()) * (fire ? 40.0f : 1.0f);
    float m2 = m1 * m1 + spread * spread;
    if (rnd() < 0.03f) m2 = nextafterf(m1 * m1, 0.0f);   // below m1 * m1 by rounding
    (*mom)[2 * i] = m1;
    (*mom)[2 * i + 1] = m2;
  }
}

void shapes() {
  const int sizes[3][2] = {{16, 16}, {37, 23}, {64, 48}};
  const uint32_t n = 2;
  for (const auto& s : sizes) {
    const int W = s[0], H = s[1];
    const size_t np = (size_t)W * H;
    float cur[16];
    orbit(0.0, cur);
    float prev[4][16];
    orbit(0.0, prev[0]);
    orbit(-2.0, prev[1]);
    camera_at(0.0f, 0.0f, 5.0f, 0.0f, 0.0f, 1.0f, prev[2]);   // looking away: z <= 0 everywhere
    orbit(-60.0, prev[3]);
    std::vector<float> c, m, g, hc, hm, hg, hl(np);
    colours(W, H, &c, &m);
    plane_guide(cur, W, H, &g);
    for (int y = H / 4; y < H / 4 + H / 3; ++y)
      for (int x = W / 4; x < W / 4 + W / 3; ++x) {
        float* p = &g[4 * ((size_t)y * W + x)];
        p[0] = p[1] = p[2] = 0.0f, p[3] = 1e30f;
      }
    std::vector<float> oc(np * 4), om(np * 2), ol(np), ov(np), filtered(np * 4);
    for (int k = 0; k < 5; ++k) {   // k == 4: no history
      pt_reproject_images im = {c.data(), m.data(), g.data(), nullptr, nullptr, nullptr, nullptr,
                                oc.data(), om.data(), ol.data(), ov.data()};
      const float* pc = prev[k < 4 ? k : 0];
      if (k < 4) {
        colours(W, H, &hc, &hm);
        plane_guide(pc, W, H, &hg);
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            float* p = &hg[4 * i];
            if (y >= 3 * H / 4) p[3] *= 1.2f;
            if (x >= 3 * W / 4 && p[3] < 1e30f) p[0] = 0.6f, p[1] = 0.8f, p[2] = 0.0f;
            hl[i] = (float)(1 + (int)(200.0f * rnd()));
            if (y >= H / 8 && y < H / 8 + H / 4 && x >= W / 2 && x < W / 2 + W / 4) hl[i] = 0.0f;
          }
        im.hist_color = hc.data(), im.hist_moments = hm.data(), im.hist_length = hl.data(), im.hist_guide = hg.data();
      }
      expect(pt_reproject_host(cur, pc, W, H, n, &im, nullptr) == PT_OK, "reproject call");
      bool finite = true, alpha = true, lens = true, same = true;
      size_t with_history = 0;
      for (size_t i = 0; i < np; ++i) {
        for (int q = 0; q < 4; ++q) finite = finite && isfinite(oc[4 * i + q]);
        finite = finite && isfinite(om[2 * i]) && isfinite(om[2 * i + 1]) && isfinite(ov[i]) && ov[i] >= 0.0f;
        alpha = alpha && memcmp(&oc[4 * i + 3], &c[4 * i + 3], 4) == 0;
        lens = lens && ol[i] >= (float)n && ol[i] <= 64.0f + (float)n && ol[i] == floorf(ol[i]);
        if (ol[i] > (float)n) ++with_history;
        if (ol[i] == (float)n) same = same && memcmp(&oc[4 * i], &c[4 * i], 16) == 0 && memcmp(&om[2 * i], &m[2 * i], 8) == 0;
      }
      expect(finite, "reprojected images finite, variance >= 0");
      expect(alpha, "alpha passes through");
      expect(lens, "lengths are whole numbers within n .. max_history + n");
      expect(same, "a pixel without history is the new frame's");
      if (k == 0 || k == 1) expect(with_history > 0, "some pixels find history");
      if (k == 2 || k == 4) expect(with_history == 0, "no pixel finds history");
      expect(pt_denoise_var_plane_host(oc.data(), ov.data(), g.data(), W, H, nullptr, filtered.data()) == PT_OK, "filter call");
      bool ff = true;
      for (size_t i = 0; i < filtered.size(); ++i) ff = ff && isfinite(filtered[i]);
      expect(ff, "filtered image finite");
    }
    // arguments
    pt_reproject_images im = {c.data(), m.data(), g.data(), hc.data(), hm.data(), hl.data(), hg.data(),
                              oc.data(), om.data(), ol.data(), ov.data()};
    expect(pt_reproject_host(cur, cur, W, H, 0, &im, nullptr) == PT_ERR_INVALID, "n = 0");
    expect(pt_reproject_host(cur, cur, W, H, 65537, &im, nullptr) == PT_ERR_INVALID, "n > 65536");
    expect(pt_reproject_host(cur, cur, 0, H, n, &im, nullptr) == PT_ERR_INVALID, "size");
    expect(pt_reproject_host(nullptr, cur, W, H, n, &im, nullptr) == PT_ERR_INVALID, "null camera");
    pt_reproject_images part = im;
    part.hist_length = nullptr;
    expect(pt_reproject_host(cur, cur, W, H, n, &part, nullptr) == PT_ERR_INVALID, "three history images");
    pt_reproject_images alias = im;
    alias.out_color = c.data();
    expect(pt_reproject_host(cur, cur, W, H, n, &alias, nullptr) == PT_ERR_INVALID, "output aliases an input");
    const pt_temporal_params bad[4] = {{0, 0.0f, 0.5f, 0.05f}, {64, 1.5f, 0.5f, 0.05f}, {64, 0.0f, -2.0f, 0.05f},
                                       {64, 0.0f, 0.5f, 0.0f}};
    for (const auto& b : bad) expect(pt_reproject_host(cur, cur, W, H, n, &im, &b) == PT_ERR_INVALID, "bad params");
    expect(pt_denoise_var_plane_host(oc.data(), nullptr, g.data(), W, H, nullptr, filtered.data()) == PT_ERR_INVALID, "null plane");
  }
}

}  // namespace

int main() {
  shapes();
  if (fails) return 1;
  printf("ok: pt_reproject_host and pt_denoise_var_plane_host on 3 shapes x (4 previous cameras + no history)\n");
  return 0;
}
