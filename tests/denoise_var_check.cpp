// Test infrastructure: a stand-alone host program around pt_denoise_var_host
// and the moments' fold (csrc/pt_denoise.h, compiled for the host), on the
// shapes the tests use -- for sanitizer runs on the CPU:
//
//   S="-O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off \
//      -fno-fast-math -D__HIP_PLATFORM_AMD__ -Iinclude -Idiscovering-path-tracer_amd/csrc"
//   for f in tests/denoise_var_check.cpp discovering-path-tracer_amd/csrc/*.cpp \
//            discovering-path-tracer_amd/csrc/scene/*.cpp; do
//     hipcc $S -c $f -o san/$(basename $f .cpp).o; done          # host objects, instrumented
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined san/*.o \
//     discovering-path-tracer_amd/build/pt_device.o discovering-path-tracer_amd/build/pt_denoise.o \
//     -lpthread -o denoise_var_check && ./denoise_var_check
//
// (the host code under test carries the instrumentation; the program calls
// nothing that touches a GPU, and it is run on the CPU only).
// tests/test_denoise_var.py builds it plainly against libptamd.so and runs it.
// It filters seeded images -- fireflies, a zero-variance block, misses in the
// guide, m2 < m1 * m1 -- at 16x16, 37x23 and 64x48 with 1, 3 and 5 passes,
// folds eight batches of sample colours into moments at 64x48 and 67x45 with
// the kernels' statements, and checks that everything is finite, that alpha
// passes through, that the moments satisfy m2 >= 0 and that bad arguments are
// refused.  Exit status 0 and one "ok" line, or 1 and what failed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pathtracer.h"
#include "pt_denoise.h"

namespace {

uint32_t g_state = 12345u;
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

void make_images(int W, int H, std::vector<float>* rgba, std::vector<float>* mom, std::vector<float>* guide) {
  const size_t n = (size_t)W * H;
  rgba->assign(n * 4, 0.0f);
  mom->assign(n * 2, 0.0f);
  guide->assign(n * 4, 0.0f);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      float* c = &(*rgba)[4 * i];
      const bool fire = rnd() < 0.05f;
      for (int k = 0; k < 3; ++k) c[k] = 2.0f * rnd() * (fire ? 40.0f : 1.0f);
      c[3] = 0.5f + 0.5f * rnd();
      const bool flat = y >= H / 2 && y < H / 2 + H / 3 && x >= W / 8 && x < W / 8 + W / 3;
      if (flat) c[0] = 0.25f, c[1] = 0.5f, c[2] = 0.75f;
      const float m1 = ptdn::lum(c[0], c[1], c[2]);
      const float spread = flat ? 0.0f : (0.05f + 1.45f * rnd()) * (fire ? 40.0f : 1.0f);
      float m2 = m1 * m1 + spread * spread;
      if (rnd() < 0.03f) m2 = nextafterf(m1 * m1, 0.0f);   // below m1 * m1 by rounding
      (*mom)[2 * i] = m1;
      (*mom)[2 * i + 1] = m2;
      float* g = &(*guide)[4 * i];
      const bool miss = y >= H / 4 && y < H / 4 + H / 3 && x >= W / 4 && x < W / 4 + W / 3;
      g[0] = miss ? 0.0f : (x >= W / 2 ? 0.6f : 0.0f);
      g[1] = 0.0f;
      g[2] = miss ? 0.0f : (x >= W / 2 ? 0.8f : 1.0f);
      g[3] = miss ? 1e30f : 3.0f + 0.01f * rnd() + (y >= H / 2 ? 0.75f : 0.0f);
    }
}

void filter_shapes() {
  const int shapes[3][2] = {{16, 16}, {37, 23}, {64, 48}};
  const int passes[3] = {1, 3, 5};
  for (const auto& s : shapes) {
    const int W = s[0], H = s[1];
    std::vector<float> rgba, mom, guide;
    make_images(W, H, &rgba, &mom, &guide);
    std::vector<float> out((size_t)W * H * 4);
    for (int it : passes) {
      const pt_denoise_var_params p = {it, 1.5f, 0.35f, 0.25f};
      expect(pt_denoise_var_host(rgba.data(), mom.data(), 8, guide.data(), W, H, &p, out.data()) == PT_OK, "filter call");
      bool finite = true, alpha = true;
      for (size_t i = 0; i < out.size(); ++i) {
        finite = finite && isfinite(out[i]);
        if (i % 4 == 3) alpha = alpha && memcmp(&out[i], &rgba[i], 4) == 0;
      }
      expect(finite, "filtered image finite");
      expect(alpha, "alpha passes through");
    }
    expect(pt_denoise_var_host(rgba.data(), mom.data(), 8, guide.data(), W, H, nullptr, out.data()) == PT_OK, "defaults");
    expect(pt_denoise_var_host(rgba.data(), mom.data(), 1, guide.data(), W, H, nullptr, out.data()) == PT_ERR_INVALID, "n < 2");
    expect(pt_denoise_var_host(nullptr, mom.data(), 8, guide.data(), W, H, nullptr, out.data()) == PT_ERR_INVALID, "null");
    expect(pt_denoise_var_host(rgba.data(), mom.data(), 8, guide.data(), 0, H, nullptr, out.data()) == PT_ERR_INVALID, "size");
    const pt_denoise_var_params bad = {7, 1.5f, 0.35f, 0.25f};
    expect(pt_denoise_var_host(rgba.data(), mom.data(), 8, guide.data(), W, H, &bad, out.data()) == PT_ERR_INVALID, "params");
  }
}

// The render kernels' fold of L and L * L (render_kernel, wf_fold_kernel), batch by batch.
void fold_shapes() {
  const int shapes[2][2] = {{64, 48}, {67, 45}};
  for (const auto& s : shapes) {
    const size_t n = (size_t)s[0] * s[1];
    std::vector<float> mom(n * 2, 0.0f);
    for (uint32_t batch = 0; batch < 8; ++batch)
      for (size_t i = 0; i < n; ++i) {
        const bool culled = i % 7 == 0;
        const float L = culled ? ptdn::lum(0.0f, 0.0f, 0.0f) : ptdn::lum(3.0f * rnd(), 3.0f * rnd(), 3.0f * rnd());
        const float fb = (float)batch, fb1 = (float)(batch + 1u);
        mom[2 * i] = (mom[2 * i] * fb + L) / fb1;
        mom[2 * i + 1] = (mom[2 * i + 1] * fb + L * L) / fb1;
      }
    bool ok = true, zeros = true;
    for (size_t i = 0; i < n; ++i) {
      const float v = ptdn::var_of_mean(mom[2 * i], mom[2 * i + 1], 8);
      ok = ok && isfinite(v) && v >= 0.0f && mom[2 * i + 1] >= 0.0f;
      if (i % 7 == 0) zeros = zeros && mom[2 * i] == 0.0f && mom[2 * i + 1] == 0.0f && !signbit(mom[2 * i]);
    }
    expect(ok, "moments finite, variance >= 0");
    expect(zeros, "culled pixels keep +0 moments");
  }
}

}  // namespace

int main() {
  filter_shapes();
  fold_shapes();
  if (fails) return 1;
  printf("ok: pt_denoise_var_host on 3 shapes x 3 pass counts, the moments' fold on 2 shapes\n");
  return 0;
}
