// pt_display.h — the display transform: exposure, tone map and the 8-bit sRGB
// encode of a W x H float4 image, and the metering pass behind auto exposure,
// stated once for the device kernels (pt_display.hip) and the host
// (pt_display_host in pt_display.cpp, tests/display_check.cpp), the way
// pt_denoise.h is: both run these statements, compiled with -ffp-contract=off,
// so the device's bytes equal the host's.  Nothing is fused, every division is
// IEEE, every association is written down:
//
//   pixel (rgb; alpha is not read, the output alpha is 255)
//     v  = c * scale                     scale = exposure, or exposure * auto_scale when metering
//     v  = fmin_(fmax_(v, 0), kBound)    NaN -> 0, negatives and -0 -> zero, +inf -> kBound
//     PT_TONEMAP_CLAMP     v unchanged (the reference's sRGB swapchain)
//     PT_TONEMAP_REINHARD  L  = lum(v);  Lp = (L * (1 + L / (white * white))) / (1 + L)
//                          v  = v * (Lp / L) when L > 0, else unchanged
//     PT_TONEMAP_ACES      v  = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f) per channel
//     code = srgb8_code(v) per channel; the word is r | g << 8 | b << 16 | 255 << 24
//
// kBound = 2^40.  Every operator is past code 255 long before it (ACES tends to
// 2.51 / 2.43, Reinhard to L / white^2 per unit of v), so clamping there changes
// no code, and it keeps the intermediates finite: the largest of ACES is
// x * (2.51 x + 0.03) < 2^82, lum(v) <= 2^40 (1 + 2^-22), and Reinhard's
// L * (1 + L / white^2) stays below 2^128 for every white >= 2^-23.  A smaller
// white is a valid parameter (its square is a non-zero float) and its quotient
// may overflow: the lit channels of a pixel then go to +inf and code 255, its
// zero channels through 0 * inf = NaN to code 0, on the device and the host alike.
//
//   srgb8_code(v): the number of thresholds kSrgb8T[1..255] that are <= v; anything
//   not > 0 (NaN included) gives 0.  kSrgb8T[k] is the least float x with
//   srgb8_pow(x) >= k, srgb8_pow being the double-precision statement
//   pt_write_image has always encoded with (below).  The table was generated once
//   from it by bisection; tests/display_check.cpp compares srgb8_code with
//   srgb8_pow for all 2^32 bit patterns, which also proves that srgb8_pow is
//   monotone (were it not, no table of thresholds could reproduce it and the
//   check would fail).  The two branches of srgb8_pow meet at 0.0031308f:
//   12.92 * x there is 0.04045, the power branch 0.04045 too, both code 10
//   (10.31 + 0.5 truncated), and kSrgb8T[10] < 0.0031308f < kSrgb8T[11].
//   The search is eight compare steps over the bit patterns (positive floats
//   order as their bits do); the kernel runs them on a copy of the table in LDS.
//
//   metering: the log-average luminance of the source
//     metered pixel   L = lum(fmax_(c.r, 0), fmax_(c.g, 0), fmax_(c.b, 0)) is finite and > 0
//     term            log_(L) of a metered pixel, +0 of any other and of a lane outside the frame
//     stage one       per 16x16 tile, lane i = ly * 16 + lx: tree256 of the 256 terms
//     stage two       lane j = 0..255 adds the tile partials j, j + 256, j + 512, ... in that
//                     order (from +0), then tree256 of the 256 lane values
//     tree256         for s = 128, 64, .., 1: v[i] += v[i + s] for every i < s
//     n               the metered pixels, counted exactly in uint32
//     result          mean = sum / float(n);  target = key / exp_(mean)
//                     scale = target without a previous scale or with adapt == 1,
//                             else prev + (target - prev) * adapt
//                     n == 0: the previous scale stands; without one, 1
//   The scale a metering call used is the next call's previous scale.
#pragma once
#include <math.h>

#include "pt_denoise.h"

namespace ptdp {
using namespace ptm;

constexpr int kClamp = 0, kReinhard = 1, kAces = 2;   // PT_TONEMAP_* (include/pathtracer.h)
constexpr float kBound = 0x1p40f;

// linear -> 8-bit sRGB after clamping to [0,1]: what an sRGB swapchain shows
// for the reference's RGBA32F image (VulkanRenderer copies it to a texture
// that color_frag.frag outputs unchanged).  Host only: the statement the
// thresholds below were generated from.
inline unsigned char srgb8_pow(float x) {
  if (!(x > 0.0f)) return 0;
  if (x >= 1.0f) return 255;
  const double e = x <= 0.0031308f ? 12.92 * x : 1.055 * pow((double)x, 1.0 / 2.4) - 0.055;
  return (unsigned char)(e * 255.0 + 0.5);
}

// kSrgb8T[k], k = 1..255: the bits of the least float with srgb8_pow >= k; [0] is +0.
#if defined(__HIP_DEVICE_COMPILE__)
__device__
#endif
static constexpr uint32_t kSrgb8T[256] = {
    0x00000000u, 0x391f22b4u, 0x39eeb40eu, 0x3a46eb61u, 0x3a8b3e5eu, 0x3ab3070bu, 0x3adacfb8u, 0x3b014c33u,
    0x3b153089u, 0x3b2914dfu, 0x3b3cf936u, 0x3b50f2d1u, 0x3b65fb9bu, 0x3b7c3403u, 0x3b89d060u, 0x3b962333u,
    0x3ba314bdu, 0x3bb0a731u, 0x3bbedcb7u, 0x3bcdb76du, 0x3bdd3967u, 0x3bed64afu, 0x3bfe3b46u, 0x3c07df91u,
    0x3c10f91bu, 0x3c1a6b32u, 0x3c2436c8u, 0x3c2e5cc7u, 0x3c38de1au, 0x3c43bba4u, 0x3c4ef648u, 0x3c5a8ee4u,
    0x3c668654u, 0x3c72dd71u, 0x3c7f950fu, 0x3c865702u, 0x3c8d148fu, 0x3c940396u, 0x3c9b247cu, 0x3ca277a6u,
    0x3ca9fd78u, 0x3cb1b653u, 0x3cb9a298u, 0x3cc1c2a9u, 0x3cca16e3u, 0x3cd29fa4u, 0x3cdb5d4bu, 0x3ce45032u,
    0x3ced78b5u, 0x3cf6d72eu, 0x3d0035fcu, 0x3d051bb4u, 0x3d0a1cecu, 0x3d0f39d0u, 0x3d14728au, 0x3d19c745u,
    0x3d1f382cu, 0x3d24c567u, 0x3d2a6f22u, 0x3d303584u, 0x3d3618b7u, 0x3d3c18e4u, 0x3d423632u, 0x3d4870cau,
    0x3d4ec8d2u, 0x3d553e73u, 0x3d5bd1d3u, 0x3d628318u, 0x3d69526au, 0x3d703feeu, 0x3d774bcau, 0x3d7e7624u,
    0x3d82df90u, 0x3d869372u, 0x3d8a56cbu, 0x3d8e29abu, 0x3d920c27u, 0x3d95fe4fu, 0x3d9a0035u, 0x3d9e11ecu,
    0x3da23384u, 0x3da66510u, 0x3daaa6a0u, 0x3daef847u, 0x3db35a15u, 0x3db7cc1bu, 0x3dbc4e6bu, 0x3dc0e114u,
    0x3dc58429u, 0x3dca37b9u, 0x3dcefbd6u, 0x3dd3d08fu, 0x3dd8b5f5u, 0x3dddac19u, 0x3de2b30au, 0x3de7cad9u,
    0x3decf395u, 0x3df22d50u, 0x3df77817u, 0x3dfcd3fcu, 0x3e012087u, 0x3e03dfaeu, 0x3e06a77bu, 0x3e0977f6u,
    0x3e0c5126u, 0x3e0f3314u, 0x3e121dc5u, 0x3e151143u, 0x3e180d95u, 0x3e1b12c2u, 0x3e1e20d1u, 0x3e2137cbu,
    0x3e2457b6u, 0x3e278099u, 0x3e2ab27du, 0x3e2ded68u, 0x3e313161u, 0x3e347e70u, 0x3e37d49cu, 0x3e3b33ecu,
    0x3e3e9c67u, 0x3e420e15u, 0x3e4588fbu, 0x3e490d22u, 0x3e4c9a90u, 0x3e50314cu, 0x3e53d15du, 0x3e577acau,
    0x3e5b2d9au, 0x3e5ee9d4u, 0x3e62af7eu, 0x3e667e9fu, 0x3e6a573eu, 0x3e6e3962u, 0x3e722511u, 0x3e761a52u,
    0x3e7a192cu, 0x3e7e21a5u, 0x3e8119e2u, 0x3e8327c7u, 0x3e853a86u, 0x3e875222u, 0x3e896e9du, 0x3e8b8ffcu,
    0x3e8db641u, 0x3e8fe170u, 0x3e92118bu, 0x3e944696u, 0x3e968095u, 0x3e98bf89u, 0x3e9b0377u, 0x3e9d4c62u,
    0x3e9f9a4cu, 0x3ea1ed38u, 0x3ea4452bu, 0x3ea6a226u, 0x3ea9042eu, 0x3eab6b44u, 0x3eadd76du, 0x3eb048aau,
    0x3eb2bf00u, 0x3eb53a71u, 0x3eb7bb00u, 0x3eba40b1u, 0x3ebccb85u, 0x3ebf5b81u, 0x3ec1f0a7u, 0x3ec48af9u,
    0x3ec72a7cu, 0x3ec9cf32u, 0x3ecc791eu, 0x3ecf2842u, 0x3ed1dca2u, 0x3ed49641u, 0x3ed75521u, 0x3eda1946u,
    0x3edce2b2u, 0x3edfb168u, 0x3ee2856au, 0x3ee55ebdu, 0x3ee83d63u, 0x3eeb215du, 0x3eee0ab1u, 0x3ef0f95fu,
    0x3ef3ed6bu, 0x3ef6e6d8u, 0x3ef9e5a8u, 0x3efce9deu, 0x3efff37eu, 0x3f018145u, 0x3f030b82u, 0x3f049877u,
    0x3f062827u, 0x3f07ba92u, 0x3f094fb9u, 0x3f0ae79fu, 0x3f0c8244u, 0x3f0e1faau, 0x3f0fbfd2u, 0x3f1162beu,
    0x3f13086eu, 0x3f14b0e4u, 0x3f165c22u, 0x3f180a29u, 0x3f19bafau, 0x3f1b6e96u, 0x3f1d24ffu, 0x3f1ede36u,
    0x3f209a3cu, 0x3f225913u, 0x3f241abcu, 0x3f25df38u, 0x3f27a689u, 0x3f2970afu, 0x3f2b3dadu, 0x3f2d0d83u,
    0x3f2ee032u, 0x3f30b5bdu, 0x3f328e24u, 0x3f346968u, 0x3f36478bu, 0x3f38288fu, 0x3f3a0c73u, 0x3f3bf33au,
    0x3f3ddce5u, 0x3f3fc975u, 0x3f41b8ebu, 0x3f43ab48u, 0x3f45a08fu, 0x3f4798bfu, 0x3f4993dbu, 0x3f4b91e3u,
    0x3f4d92d8u, 0x3f4f96bdu, 0x3f519d92u, 0x3f53a758u, 0x3f55b411u, 0x3f57c3beu, 0x3f59d65fu, 0x3f5bebf7u,
    0x3f5e0486u, 0x3f60200eu, 0x3f623e90u, 0x3f64600cu, 0x3f668485u, 0x3f68abfbu, 0x3f6ad670u, 0x3f6d03e5u,
    0x3f6f345au, 0x3f7167d2u, 0x3f739e4du, 0x3f75d7ccu, 0x3f781451u, 0x3f7a53ddu, 0x3f7c9671u, 0x3f7edc0eu,
};

// The count of thresholds <= v in a table T[0..255] (T[0] = 0) by eight compare steps.
template <class Table>
PT_FN uint32_t srgb8_search(const Table& T, float v) {
  if (!(v > 0.0f)) return 0u;
  const uint32_t u = f2u(v);
  uint32_t k = 0u;
  for (uint32_t s = 128u; s > 0u; s >>= 1)
    if (T[k + s] <= u) k += s;
  return k;
}
PT_FN uint32_t srgb8_code(float v) { return srgb8_search(kSrgb8T, v); }

PT_FN float range_(float v) { return fmin_(fmax_(v, 0.0f), kBound); }

PT_FN float aces_(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

// What a pixel needs of pt_display_params: the operator, the scale and white * white.
struct Tone {
  int tonemap;
  float scale, w2;
};

// rgb of one pixel before the encode.
PT_FN void tone_pixel(float4 c, Tone t, float* r, float* g, float* b) {
  float x = range_(c.x * t.scale), y = range_(c.y * t.scale), z = range_(c.z * t.scale);
  if (t.tonemap == kReinhard) {
    const float L = ptdn::lum(x, y, z);
    if (L > 0.0f) {
      const float Lp = (L * (1.0f + L / t.w2)) / (1.0f + L);
      const float q = Lp / L;
      x = x * q;
      y = y * q;
      z = z * q;
    }
  } else if (t.tonemap == kAces) {
    x = aces_(x);
    y = aces_(y);
    z = aces_(z);
  }
  *r = x;
  *g = y;
  *b = z;
}

// One pixel: the packed RGBA8 word.
template <class Table>
PT_FN uint32_t display_pixel(const Table& T, float4 c, Tone t) {
  float r, g, b;
  tone_pixel(c, t, &r, &g, &b);
  return srgb8_search(T, r) | (srgb8_search(T, g) << 8) | (srgb8_search(T, b) << 16) | 0xff000000u;
}

// finite, > 0 (NaN fails both)
PT_FN bool pos_finite(float x) { return x > 0.0f && x <= 3.40282347e38f; }

PT_FN bool params_ok(int tonemap, float exposure, int auto_exposure, float key, float white, float adapt) {
  if (tonemap < kClamp || tonemap > kAces || auto_exposure < 0 || auto_exposure > 1) return false;
  if (!pos_finite(exposure) || !pos_finite(key) || !pos_finite(white) || !pos_finite(white * white)) return false;
  return adapt > 0.0f && adapt <= 1.0f;
}

// ---- metering ----------------------------------------------------------------
// A pixel's term and whether it is metered.
PT_FN float meter_term(float4 c, bool* metered) {
  const float L = ptdn::lum(fmax_(c.x, 0.0f), fmax_(c.y, 0.0f), fmax_(c.z, 0.0f));
  *metered = pos_finite(L);
  return *metered ? log_(L) : 0.0f;
}

// One step of tree256 for lane i < s (the kernels run the lanes of a step side by
// side, a barrier between steps), and the whole tree in place.
PT_FN void tree_step(float* v, int i, int s) { v[i] += v[i + s]; }
PT_FN float tree256(float* v) {
  for (int s = 128; s > 0; s >>= 1)
    for (int i = 0; i < s; ++i) tree_step(v, i, s);
  return v[0];
}

// Lane j of stage two: the tile partials j, j + 256, ... in that order.
PT_FN float meter_lane(const float* partial, int n_tiles, int j) {
  float s = 0.0f;
#pragma unroll 8   // the loads ahead of the adds; the adds stay in order
  for (int t = j; t < n_tiles; t += 256) s += partial[t];
  return s;
}

// The scale of a metering call from the sum and the count; prev is read only with have_prev.
PT_FN float meter_scale(float sum, uint32_t n, float key, float adapt, bool have_prev, float prev) {
  if (n == 0u) return have_prev ? prev : 1.0f;
  const float mean = sum / (float)n;
  const float target = key / exp_(mean);
  if (!have_prev || adapt == 1.0f) return target;
  return prev + (target - prev) * adapt;
}

// The metering state in device memory (pt_display.hip writes it, display_kernel reads scale).
struct MeterState {
  float scale;
  uint32_t n;
};

}  // namespace ptdp

namespace ptd {
// pt_display.hip.  The images are W x H in row order; dst holds one 32-bit word a pixel.
// launch_display: state null = no metering (scale = exposure), else scale = exposure * state->scale.
hipError_t launch_display(const float4* src, uint32_t* dst, size_t n_pixels, int tonemap, float exposure, float w2,
                          const ptdp::MeterState* state, hipStream_t stream);
// Both metering stages: partial_sum and partial_n hold a value per 16x16 tile; have_prev 0 = the
// state holds no previous scale.
hipError_t launch_display_meter(const float4* src, int width, int height, float* partial_sum, uint32_t* partial_n,
                                float key, float adapt, int have_prev, ptdp::MeterState* state, hipStream_t stream);
}  // namespace ptd
