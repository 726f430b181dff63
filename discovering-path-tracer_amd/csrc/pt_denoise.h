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

}  // namespace ptdn
