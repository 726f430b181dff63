// pt_denoise.h — the first-hit guide ray and the edge-avoiding a-trous filter
// (Dammertz et al., HPG 2010), stated once for the device kernels
// (guide_kernel in pt_device.hip, atrous_kernel in pt_denoise.hip) and the host
// (pt_guide_ray, pt_denoise_host in pt_api.cpp), the way wide_walk.h is
// shared with tests/wide_check.cpp: both run the same statements, compiled
// with -ffp-contract=off, so the device image equals the host's bit for bit.
//
// Every association is fixed here:
//   guide ray   ndc = ((2 * float(p)) / float(res)) - 1
//               dir = normalize((cdir + (-right) * ((ndcX * tanFov) * aspect)) - up * (ndcY * tanFov))
//   tap         d2c = (dx*dx + dy*dy) + dz*dz over rgb of c_p - c_q, d2n the same over the normals,
//               dz  = t_p - t_q
//               w   = h * exp_(-((d2c / sc2 + d2n / sn2) + (dz * dz) / sz2))
//               sum.rgb += w * c_q.rgb, sum.w += w   (one add per channel per tap)
//   pixel       taps in the order dy = -2..2 outer, dx = -2..2 inner, those
//               outside the frame skipped; out.rgb = sum.rgb / sum.w, out.a = c_p.a
// sc2 = sc * sc with sc = sigma_color * 2^-i (exact scaling) in pass i,
// sn2 = sigma_normal^2, sz2 = sigma_depth^2; h = k[|dx|] * k[|dy|] with
// k = {3/8, 1/4, 1/16}, every product exact.  One exp_ per tap: three would
// triple the filter's only expensive operation and round three times; the sum
// of the three quotients rounds twice and costs two adds.
//
// Further down: the luminance of the moments the render kernels fold
// (PT_OPT_MOMENTS) and the variance-guided filter built on them
// (atrous_var_pixel: pt_denoise_var, pt_denoise_var_host), stated the same way.
#pragma once
#include "pt_math.h"

namespace ptdn {
using namespace ptm;

constexpr int kMaxIterations = 6;

// The camera frame of main() (raytrace_comp.comp:447-448, :457) from the
// std140 camera block: pos@0, dir@4, up@8, fov@12.
struct CamBasis {
  v3 pos, dir, right, up;
  float tan_fov;
};
PT_FN CamBasis cam_basis(const float cam[16]) {
  CamBasis b;
  b.pos = mk(cam[0], cam[1], cam[2]);
  b.dir = mk(cam[4], cam[5], cam[6]);
  const v3 cup = mk(cam[8], cam[9], cam[10]);
  b.right = normalize(cross(b.dir, neg(cup)));
  b.up = normalize(cross(b.right, b.dir));
  b.tan_fov = tan_(radians_(cam[12] * 0.5f));
  return b;
}

// The pixel's centre ray: no aperture draw, no jitter (:430-432, :458).
PT_FN v3 guide_dir(v3 cdir, v3 right, v3 up, float tan_fov, int W, int H, int x, int y) {
  const float ndcX = (2.0f * (float)x / (float)W) - 1.0f;
  const float ndcY = (2.0f * (float)y / (float)H) - 1.0f;
  const float aspect = (float)W / (float)H;
  return normalize(sub(add(cdir, muls(neg(right), (ndcX * tan_fov) * aspect)), muls(up, ndcY * tan_fov)));
}

// Squared sigmas of one pass.
struct Sigma2 {
  float c, n, z;
};
PT_FN Sigma2 pass_sigma2(float sigma_color, float sigma_normal, float sigma_depth, int pass) {
  const float sc = sigma_color * u2f((uint32_t)(127 - pass) << 23);   // * 2^-pass
  Sigma2 s;
  s.c = sc * sc;
  s.n = sigma_normal * sigma_normal;
  s.z = sigma_depth * sigma_depth;
  return s;
}
// iterations 1..6, sigmas finite and > 0 -- and every pass's squared sigma a
// finite non-zero float (a zero one would make the centre tap 0 / 0).
PT_FN bool params_ok(int iterations, float sigma_color, float sigma_normal, float sigma_depth) {
  if (iterations < 1 || iterations > kMaxIterations) return false;
  const float big = 3.40282347e38f;
  if (!(sigma_color > 0.0f && sigma_color <= big && sigma_normal > 0.0f && sigma_normal <= big &&
        sigma_depth > 0.0f && sigma_depth <= big))
    return false;
  const Sigma2 s = pass_sigma2(sigma_color, sigma_normal, sigma_depth, iterations - 1);   // the smallest sc
  const Sigma2 s0 = pass_sigma2(sigma_color, sigma_normal, sigma_depth, 0);               // the largest
  return s.c > 0.0f && s0.c <= big && s.n > 0.0f && s.n <= big && s.z > 0.0f && s.z <= big;
}

PT_FN float tap_kernel(int d) {
  const int a = d < 0 ? -d : d;
  return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// One tap: colour c_q and guide g_q = {n.xyz, t} against the centre's.
PT_FN void atrous_tap(float4 cp, float4 gp, float4 cq, float4 gq, float h, Sigma2 s, float4* sum) {
  const float cx = cp.x - cq.x, cy = cp.y - cq.y, cz = cp.z - cq.z;
  const float d2c = (cx * cx + cy * cy) + cz * cz;
  const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
  const float d2n = (nx * nx + ny * ny) + nz * nz;
  const float dz = gp.w - gq.w;
  const float w = h * exp_(-((d2c / s.c + d2n / s.n) + (dz * dz) / s.z));
  sum->x += w * cq.x;
  sum->y += w * cq.y;
  sum->z += w * cq.z;
  sum->w += w;
}

// One pixel of one pass.  Fetch: void operator()(int qx, int qy, float4* c,
// float4* g) for a tap inside the frame (the plain kernel and the host read
// the images, the staged kernel its LDS tile: the same values).
template <class Fetch>
PT_FN float4 atrous_pixel(const Fetch& fetch, int W, int H, int x, int y, int step, Sigma2 s) {
  float4 cp, gp;
  fetch(x, y, &cp, &gp);
  float4 sum;
  sum.x = sum.y = sum.z = sum.w = 0.0f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + step * dy;
    if (qy < 0 || qy >= H) continue;
    const float ky = tap_kernel(dy);
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + step * dx;
      if (qx < 0 || qx >= W) continue;
      float4 cq, gq;
      fetch(qx, qy, &cq, &gq);
      atrous_tap(cp, gp, cq, gq, tap_kernel(dx) * ky, s, &sum);
    }
  }
  float4 out;
  out.x = sum.x / sum.w;
  out.y = sum.y / sum.w;
  out.z = sum.z / sum.w;
  out.w = cp.w;
  return out;
}

struct ImageFetch {
  const float4* color;
  const float4* guide;
  int W;
  __host__ __device__ inline void operator()(int qx, int qy, float4* c, float4* g) const {
    const size_t i = (size_t)qy * (size_t)W + (size_t)qx;
    *c = color[i];
    *g = guide[i];
  }
};

// ---- the variance-guided filter (pt_denoise_var) ----------------------------
// The colour edge-stop of the filter above is driven by each pixel's own
// variance of the mean instead of a fixed sigma_color (Schied et al., SVGF, HPG
// 2017), from the luminance moments the render kernels fold (PT_OPT_MOMENTS):
//   lum(r,g,b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b
//   var0_p = fmax_(0, m2_p - m1_p * m1_p) / float(n - 1)
//   pass i = 0 .. iterations-1, s = 1 << i, on colour c and variance v (v = var0 in pass 0):
//     gv_p  = (sum of (g[|dx|] * g[|dy|]) * v_q) / (sum of g[|dx|] * g[|dy|])
//             over q = p + (dx, dy), dy = -1..1 outer, dx = -1..1 inner, spacing 1,
//             taps outside the frame skipped, g = {1/2, 1/4}
//     den_p = sigma_lum * sqrt_(gv_p) + 1e-6f
//     over the 25 taps q = p + s * (dx, dy), dy outer, dx inner, outside skipped
//     (h, d2n, dz, sn2, sz2 as above):
//       w      = h * exp_(-((fabs(lum(c_p) - lum(c_q)) / den_p + d2n / sn2) + (dz * dz) / sz2))
//       sum_c += w * c_q.rgb;   sum_v += (w * w) * v_q;   sum_w += w
//     out.rgb = sum_c / sum_w,  out.a = c_p.a,  v_out = sum_v / (sum_w * sum_w)
// sigma_lum is the same in every pass: the variance shrinks by itself.
PT_FN float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

PT_FN float var_of_mean(float m1, float m2, uint32_t n) { return fmax_(0.0f, m2 - m1 * m1) / (float)(n - 1u); }

PT_FN bool var_params_ok(int iterations, float sigma_lum, float sigma_normal, float sigma_depth) {
  if (iterations < 1 || iterations > kMaxIterations) return false;
  const float big = 3.40282347e38f;
  if (!(sigma_lum > 0.0f && sigma_lum <= big && sigma_normal > 0.0f && sigma_normal <= big && sigma_depth > 0.0f &&
        sigma_depth <= big))
    return false;
  const float l2 = sigma_lum * sigma_lum, n2 = sigma_normal * sigma_normal, z2 = sigma_depth * sigma_depth;
  return l2 > 0.0f && l2 <= big && n2 > 0.0f && n2 <= big && z2 > 0.0f && z2 <= big;
}

PT_FN float var_tap_kernel(int d) { return d == 0 ? 0.5f : 0.25f; }

struct VarOut {
  float4 c;
  float v;
};

// One pixel of one pass.  Fetch: operator()(qx, qy, &c, &g, &v) for a tap inside
// the frame, and var(qx, qy) for the 3x3 prefilter's.
template <class Fetch>
PT_FN VarOut atrous_var_pixel(const Fetch& fetch, int W, int H, int x, int y, int step, float sigma_lum, float sn2,
                              float sz2) {
  float gsum = 0.0f, gw = 0.0f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= H) continue;
    const float ky = var_tap_kernel(dy);
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= W) continue;
      const float k = var_tap_kernel(dx) * ky;
      gsum += k * fetch.var(qx, qy);
      gw += k;
    }
  }
  const float den = sigma_lum * sqrt_(gsum / gw) + 1e-6f;
  float4 cp, gp;
  float vp;
  fetch(x, y, &cp, &gp, &vp);
  const float lp = lum(cp.x, cp.y, cp.z);
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f, sw = 0.0f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + step * dy;
    if (qy < 0 || qy >= H) continue;
    const float ky = tap_kernel(dy);
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + step * dx;
      if (qx < 0 || qx >= W) continue;
      float4 cq, gq;
      float vq;
      fetch(qx, qy, &cq, &gq, &vq);
      const float h = tap_kernel(dx) * ky;
      const float dl = __builtin_fabsf(lp - lum(cq.x, cq.y, cq.z));
      const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
      const float d2n = (nx * nx + ny * ny) + nz * nz;
      const float dz = gp.w - gq.w;
      const float w = h * exp_(-((dl / den + d2n / sn2) + (dz * dz) / sz2));
      sx += w * cq.x;
      sy += w * cq.y;
      sz += w * cq.z;
      sv += (w * w) * vq;
      sw += w;
    }
  }
  VarOut o;
  o.c.x = sx / sw;
  o.c.y = sy / sw;
  o.c.z = sz / sw;
  o.c.w = cp.w;
  o.v = sv / (sw * sw);
  return o;
}

struct VarImageFetch {
  const float4* color;
  const float4* guide;
  const float* variance;
  int W;
  __host__ __device__ inline void operator()(int qx, int qy, float4* c, float4* g, float* v) const {
    const size_t i = (size_t)qy * (size_t)W + (size_t)qx;
    *c = color[i];
    *g = guide[i];
    *v = variance[i];
  }
  __host__ __device__ inline float var(int qx, int qy) const { return variance[(size_t)qy * (size_t)W + (size_t)qx]; }
};

}  // namespace ptdn
