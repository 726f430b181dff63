// Test infrastructure: a stand-alone host program around the adaptive stopping
// rule's host statement (csrc/pt_denoise.h adaptive_select_image, which
// pt_adaptive_select_host runs), for sanitizer runs on the CPU.  It includes
// the header alone and links nothing of the library, so
//
//   hipcc -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -ffp-contract=off -fno-fast-math \
//         -fsanitize=address,undefined -fno-sanitize-recover=all -I discovering-path-tracer_amd/csrc \
//         tests/adaptive_check.cpp -o adaptive_check && ./adaptive_check
//
// instruments every line under test; tests/test_adaptive.py builds and runs
// exactly that.  The frame is 40x24 (3 x 2 tiles, partial on the right and at
// the bottom) in arrays of exactly W*H*2 floats and one word per tile, with no
// slack behind them: a read or write past a partial tile is an error the
// sanitizer reports.  Cases: an all-zero tile, a converged tile holding the
// clamp (m2 < m1 * m1) and means below the floor, a noisy tile, a pixel exactly
// at the threshold and one an ulp above, a NaN and an infinite moment, counts
// at max_batches, and n + step past max_batches (also with a step near 2^32).
// Exit status 0 and one "ok" line, or 1 and what failed.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "pt_denoise.h"

namespace {

int fails = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", what);
    ++fails;
  }
}

constexpr int W = 40, H = 24, TILES = 6;

std::vector<float> crafted() {
  std::vector<float> m((size_t)W * H * 2, 0.0f);
  auto at = [&m](int x, int y) { return &m[((size_t)y * W + x) * 2]; };
  uint32_t s = 2463534242u;
  auto rnd = [&s]() {   // xorshift32 -> [0, 1)
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return (float)(s >> 8) * (1.0f / 16777216.0f);
  };
  for (int y = 0; y < 16; ++y)
    for (int x = 16; x < 32; ++x) {   // tile 1: e <= 0.2 at n = 2
      const float m1 = 0.5f + 1.5f * rnd(), d = 0.2f * rnd() * m1;
      at(x, y)[0] = m1;
      at(x, y)[1] = m1 * m1 + d * d;
    }
  at(20, 3)[0] = 1.5f, at(20, 3)[1] = 2.0f;        // the clamp
  at(21, 4)[0] = 0.01f, at(21, 4)[1] = 0.0002f;    // below the floor
  for (int y = 0; y < 16; ++y)
    for (int x = 32; x < 40; ++x) {   // tile 2: e >= 0.5 at n = 2
      at(x, y)[0] = 1.0f;
      at(x, y)[1] = 1.25f + 3.0f * rnd();
    }
  at(0, 16)[0] = 1.0f, at(0, 16)[1] = 1.0625f;     // tile 3: exactly at the threshold 0.25 at n = 2
  at(18, 20)[0] = std::numeric_limits<float>::quiet_NaN();          // tile 4
  at(39, 23)[0] = 1.0f, at(39, 23)[1] = std::numeric_limits<float>::infinity();   // tile 5: the frame's last pixel
  return m;
}

}  // namespace

int main() {
  const std::vector<float> m = crafted();
  const ptdn::AdaptiveParams a = {2u, 9u, 3u, 0.25f, 0.0625f};
  {
    const std::vector<uint32_t> n(TILES, 2u);
    std::vector<uint32_t> next(TILES, 77u);
    std::vector<float> e(TILES, -1.0f);
    ptdn::adaptive_select_image(m.data(), n.data(), W, H, a, next.data(), e.data());
    const uint32_t want[TILES] = {2u, 2u, 5u, 2u, 5u, 5u};
    for (int b = 0; b < TILES; ++b) expect(next[b] == want[b], "counts from 2");
    expect(e[0] == 0.0f && !signbit(e[0]), "an all-zero tile has E = +0");
    expect(e[1] > 0.0f && e[1] <= 0.25f, "the converged tile's error is within the threshold");
    expect(e[2] >= 0.5f && isfinite(e[2]), "the noisy tile's error");
    expect(e[3] == 0.25f, "exactly at the threshold");
    expect(isinf(e[4]) && e[4] > 0.0f, "a NaN moment reports +inf");
    expect(isinf(e[5]) && e[5] > 0.0f, "an infinite moment reports +inf");
    // errors may be null; next may be the counts themselves
    std::vector<uint32_t> in_place(n);
    ptdn::adaptive_select_image(m.data(), in_place.data(), W, H, a, in_place.data(), nullptr);
    for (int b = 0; b < TILES; ++b) expect(in_place[b] == want[b], "in place, no errors");
  }
  {
    std::vector<float> m2(m);
    m2[((size_t)16 * W + 0) * 2 + 1] = nextafterf(1.0625f, 2.0f);
    const std::vector<uint32_t> n(TILES, 2u);
    std::vector<uint32_t> next(TILES);
    std::vector<float> e(TILES);
    ptdn::adaptive_select_image(m2.data(), n.data(), W, H, a, next.data(), e.data());
    expect(next[3] == 5u && e[3] > 0.25f, "an ulp above the threshold is not converged");
  }
  {
    const uint32_t n[TILES] = {9u, 9u, 9u, 9u, 9u, 9u};   // at max_batches: nothing moves
    uint32_t next[TILES];
    ptdn::adaptive_select_image(m.data(), n, W, H, a, next, nullptr);
    for (int b = 0; b < TILES; ++b) expect(next[b] == 9u, "counts at max_batches stay");
    const uint32_t n8[TILES] = {8u, 8u, 8u, 8u, 8u, 8u};  // 8 + 3 overshoots 9
    ptdn::adaptive_select_image(m.data(), n8, W, H, a, next, nullptr);
    expect(next[2] == 9u && next[4] == 9u && next[5] == 9u && next[0] == 8u, "n + step stops at max_batches");
    const ptdn::AdaptiveParams big = {2u, 9u, 0xffffffffu, 0.25f, 0.0625f};
    ptdn::adaptive_select_image(m.data(), n8, W, H, big, next, nullptr);
    expect(next[2] == 9u && next[0] == 8u, "a step near 2^32 does not wrap");
  }
  expect(!ptdn::adaptive_params_ok(1, 9, 3, 0.25f, 0.1f) && !ptdn::adaptive_params_ok(4, 3, 3, 0.25f, 0.1f) &&
             !ptdn::adaptive_params_ok(2, 9, 0, 0.25f, 0.1f) && !ptdn::adaptive_params_ok(2, 9, 3, 0.0f, 0.1f) &&
             !ptdn::adaptive_params_ok(2, 9, 3, NAN, 0.1f) && !ptdn::adaptive_params_ok(2, 9, 3, 0.25f, INFINITY) &&
             !ptdn::adaptive_params_ok(2, 9, 3, 0.25f, -1.0f) && ptdn::adaptive_params_ok(2, 2, 1, 0.25f, 0.1f),
         "parameter ranges");
  if (fails) return 1;
  printf("ok: adaptive rule on %dx%d, %d tiles\n", W, H, TILES);
  return 0;
}
