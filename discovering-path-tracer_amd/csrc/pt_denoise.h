// pt_denoise.h — the first-hit guide ray and the edge-avoiding a-trous filter
// (Dammertz et al., HPG 2010), stated once for the device kernels
// (guide_kernel in kernels/guide.h, atrous_kernel in pt_denoise.hip) and the host
// (pt_guide_ray, pt_denoise_host in pt_post.cpp), the way wide_walk.h is
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
// (atrous_var_pixel: pt_denoise_var, pt_denoise_var_host), stated the same way,
// temporal reprojection (reproject_pixel: pt_reproject, pt_reproject_host) and
// the spatial variance estimate of pixels with a short history
// (spatial_var_pixel: pt_spatial_variance, pt_spatial_variance_host), and
// last the stopping rule of adaptive sampling (adaptive_error, adaptive_next:
// pt_adaptive_select, pt_adaptive_select_host).
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
//   var0_p = fmax_(0, m2_p - m1_p * m1_p) / float(n - 1)      (fmax_(0, x) here and below: clamp0_, x > 0 ? x : +0)
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

// The clamp of a variance at zero, the fmax_(0, x) of the statements: x where x > 0, else +0 -- for a NaN (as
// maxNum gives) and for -0, which m2 = -0 beside m1 = +-0 produces.  maxNum may return either zero for (+0, -0),
// and the host's compile of fmax_ did: -0 at one call site, +0 at another.  A comparison has one answer everywhere.
PT_FN float clamp0_(float x) { return x > 0.0f ? x : 0.0f; }

PT_FN float var_of_mean(float m1, float m2, uint32_t n) { return clamp0_(m2 - m1 * m1) / (float)(n - 1u); }

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

// ---- temporal reprojection (pt_reproject, pt_temporal_advance) --------------
// SVGF's first stage: the new frame c (n samples, moments m, guide g = {n.xyz, t}
// from camera B) is blended with the history (colour hc, moments hm, length hl
// in samples, guide hg, all from camera Bp) found where the pixel's first hit
// projects into the previous frame.  Per pixel p = (x, y):
//   no history (out = c, out_m = m, out_len = float(n)) if any "else none" applies
//   t = g_p.w;  if !(t < 1e30f) none                                   (a miss)
//   P = add(B.pos, muls(guide_dir(B.dir, B.right, B.up, B.tan_fov, W, H, x, y), t))
//   v = sub(P, Bp.pos);  z = dot(v, Bp.dir);  if !(z > 0) none
//   aspect = float(W) / float(H)
//   sx = dot(v, neg(Bp.right)) / (z * (Bp.tan_fov * aspect));   sy = dot(v, neg(Bp.up)) / (z * Bp.tan_fov)
//   fx = ((sx + 1) * float(W)) * 0.5f;   fy = ((sy + 1) * float(H)) * 0.5f
//   if !(fx > -1 && fx < float(W) && fy > -1 && fy < float(H)) none     (also NaN)
//   x0f = floor_(fx), ax = fx - x0f, x0 = int(x0f);  y likewise;  dexp = length(v)
//   taps q = (x0 + tx, y0 + ty), ty = 0..1 outer, tx = 0..1 inner, outside the frame skipped:
//     b = (tx ? ax : 1 - ax) * (ty ? ay : 1 - ay)
//     valid iff hl_q > 0 && hg_q.w < 1e30f && fabs_(hg_q.w - dexp) <= depth_rel * dexp
//               && dot(g_p.xyz, hg_q.xyz) >= normal_min
//     valid: sw += b;  sc.rgb += b * hc_q.rgb;  sm += b * hm_q;  lmin = fmin_(lmin, hl_q)
//   if !(sw > 0) none
//   h = sc / sw;  h_m = sm / sw;  N = fmin_(lmin, float(max_history))
//   a = fmax_(alpha_min, float(n) / (N + float(n)))
//   out.rgb = h + (c.rgb - h) * a;  out.a = c.a;  out_m = h_m + (m - h_m) * a;  out_len = N + float(n)
//   always   out_var = fmax_(0, out_m.y - out_m.x * out_m.x) / fmax_(out_len - 1, 1)
// t is a distance along a unit ray, so dexp is the distance the previous guide
// should hold at that point; the guide ray passes through integer pixel
// coordinates (ndc = 2x/W - 1), hence no half-pixel offset.  lmin starts at
// +inf.  n and max_history are at most 65536: every length is an exact float.
struct TemporalParams {
  float max_history;   // float(max_history)
  float alpha_min, normal_min, depth_rel;
};
PT_FN bool temporal_params_ok(uint32_t max_history, float alpha_min, float normal_min, float depth_rel) {
  return max_history >= 1u && max_history <= 65536u && alpha_min >= 0.0f && alpha_min <= 1.0f && normal_min >= -1.0f &&
         normal_min <= 1.0f && depth_rel > 0.0f && depth_rel <= 3.40282347e38f;
}

// The history images; color null: no history.
struct HistImages {
  const float4* color;
  const float2* moments;
  const float* length;
  const float4* guide;
};

struct ReprojOut {
  float4 c;
  float2 m;
  float len, var;
};

PT_FN ReprojOut reproject_pixel(const HistImages& hist, const CamBasis& B, const CamBasis& Bp, int W, int H, int x,
                                int y, float4 c, float2 m, float4 g, float fn, TemporalParams tp) {
  ReprojOut o;
  o.c = c;
  o.m = m;
  o.len = fn;
  bool found = false;
  float3 sc = {0.0f, 0.0f, 0.0f};
  float2 sm = {0.0f, 0.0f};
  float sw = 0.0f, lmin = u2f(0x7f800000u);
  const float t = g.w;
  if (hist.color && t < 1e30f) {
    const v3 P = add(B.pos, muls(guide_dir(B.dir, B.right, B.up, B.tan_fov, W, H, x, y), t));
    const v3 v = sub(P, Bp.pos);
    const float z = dot(v, Bp.dir);
    if (z > 0.0f) {
      const float aspect = (float)W / (float)H;
      const float sx = dot(v, neg(Bp.right)) / (z * (Bp.tan_fov * aspect));
      const float sy = dot(v, neg(Bp.up)) / (z * Bp.tan_fov);
      const float fx = ((sx + 1.0f) * (float)W) * 0.5f;
      const float fy = ((sy + 1.0f) * (float)H) * 0.5f;
      if (fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {
        const float x0f = floor_(fx), y0f = floor_(fy);
        const float ax = fx - x0f, ay = fy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;
        const float dexp = length(v);
        const float dtol = tp.depth_rel * dexp;
        const v3 np = mk(g.x, g.y, g.z);
        for (int ty = 0; ty < 2; ++ty) {
          const int qy = y0 + ty;
          if (qy < 0 || qy >= H) continue;
          const float by = ty ? ay : 1.0f - ay;
          for (int tx = 0; tx < 2; ++tx) {
            const int qx = x0 + tx;
            if (qx < 0 || qx >= W) continue;
            const float b = (tx ? ax : 1.0f - ax) * by;
            const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
            const float hl = hist.length[q];
            const float4 hg = hist.guide[q];
            if (hl > 0.0f && hg.w < 1e30f && fabs_(hg.w - dexp) <= dtol && dot(np, mk(hg.x, hg.y, hg.z)) >= tp.normal_min) {
              const float4 hc = hist.color[q];
              const float2 hm = hist.moments[q];
              sw += b;
              sc.x += b * hc.x;
              sc.y += b * hc.y;
              sc.z += b * hc.z;
              sm.x += b * hm.x;
              sm.y += b * hm.y;
              lmin = fmin_(lmin, hl);
            }
          }
        }
        found = sw > 0.0f;
      }
    }
  }
  if (found) {
    const float hx = sc.x / sw, hy = sc.y / sw, hz = sc.z / sw;
    const float hm1 = sm.x / sw, hm2 = sm.y / sw;
    const float N = fmin_(lmin, tp.max_history);
    const float a = fmax_(tp.alpha_min, fn / (N + fn));
    o.c.x = hx + (c.x - hx) * a;
    o.c.y = hy + (c.y - hy) * a;
    o.c.z = hz + (c.z - hz) * a;
    o.m.x = hm1 + (m.x - hm1) * a;
    o.m.y = hm2 + (m.y - hm2) * a;
    o.len = N + fn;
  }
  o.var = clamp0_(o.m.y - o.m.x * o.m.x) / fmax_(o.len - 1.0f, 1.0f);
  return o;
}

// ---- spatial variance of short histories (pt_spatial_variance) --------------
// SVGF's variance estimation stage: a pixel whose history is shorter than
// `below` samples has no usable variance of its own (one sample: m2 == m1 * m1,
// out_var above is 0), so it takes the variance of the moments pooled over its
// neighbourhood under the geometric edge-stops.  Per pixel p, from moments m,
// length len (>= 1), variance var and guide g = {n.xyz, t}:
//   if !(len_p < float(below))  out_p = var_p                       (the same bits)
//   else over q = p + (dx, dy), dy = -r..r outer, dx = -r..r inner, taps outside
//   the frame skipped, the centre included:
//     d2n = (dnx*dnx + dny*dny) + dnz*dnz  (normals of g_p - g_q);  dz = g_p.w - g_q.w
//     w   = exp_(-(d2n / sn2 + (dz * dz) / sz2)) * len_q
//     sw += w;  s1 += w * m_q.x;  s2 += w * m_q.y
//   M1 = s1 / sw;  M2 = s2 / sw;  out_p = fmax_(0, M2 - M1 * M1) / len_p
// sn2 = sigma_normal^2, sz2 = sigma_depth^2.  The centre tap weighs len_p >= 1,
// so sw > 0 for finite input; a hit next to a miss has dz * dz = inf, w = 0; two
// misses pool their zero moments.  A tap weighs its sample count, which makes
// M2 - M1 * M1 the pooled per-sample variance; / len_p: that of p's mean.
constexpr int kMaxSpatialRadius = 3;

PT_FN bool spatial_params_ok(uint32_t below, int radius, float sigma_normal, float sigma_depth) {
  if (below > 65536u || radius < 1 || radius > kMaxSpatialRadius) return false;
  const float big = 3.40282347e38f;
  if (!(sigma_normal > 0.0f && sigma_normal <= big && sigma_depth > 0.0f && sigma_depth <= big)) return false;
  const float n2 = sigma_normal * sigma_normal, z2 = sigma_depth * sigma_depth;
  return n2 > 0.0f && n2 <= big && z2 > 0.0f && z2 <= big;
}

// One short pixel (the caller has tested len_p < below).  Fetch:
// operator()(qx, qy, &m, &len, &g) for a tap inside the frame.
template <class Fetch>
PT_FN float spatial_var_pixel(const Fetch& fetch, int W, int H, int x, int y, int r, float sn2, float sz2, float4 gp,
                              float lenp) {
  float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
  for (int dy = -r; dy <= r; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= H) continue;
    for (int dx = -r; dx <= r; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= W) continue;
      float2 mq;
      float lq;
      float4 gq;
      fetch(qx, qy, &mq, &lq, &gq);
      const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
      const float d2n = (nx * nx + ny * ny) + nz * nz;
      const float dz = gp.w - gq.w;
      // a tap whose guide equals the centre's (the centre itself; a miss beside a miss -- and misses never find
      // history, so a frame's background stays short): d2n = dz = 0, the argument is -0, exp_(-0) is 1 and
      // 1 * len_q is len_q -- the statement's bits for finite guides, without the exp_ and the two divisions
      float w = lq;
      if (!(gp.x == gq.x && gp.y == gq.y && gp.z == gq.z && gp.w == gq.w))
        w = exp_(-(d2n / sn2 + (dz * dz) / sz2)) * lq;
      sw += w;
      s1 += w * mq.x;
      s2 += w * mq.y;
    }
  }
  const float M1 = s1 / sw, M2 = s2 / sw;
  return clamp0_(M2 - M1 * M1) / lenp;
}

struct SpatialImageFetch {
  const float2* moments;
  const float* length;
  const float4* guide;
  int W;
  __host__ __device__ inline void operator()(int qx, int qy, float2* m, float* l, float4* g) const {
    const size_t i = (size_t)qy * (size_t)W + (size_t)qx;
    *m = moments[i];
    *l = length[i];
    *g = guide[i];
  }
};

// ---- adaptive sampling: the stopping rule (pt_adaptive_select) ---------------
// Per 16x16 tile (raster order) with count n and each of its pixels p inside
// the frame, from the moments {m1, m2}:
//   finite_p = fabs(m1_p) <= FLT_MAX && fabs(m2_p) <= FLT_MAX
//   e_p = finite_p ? sqrt_(var_of_mean(m1_p, m2_p, n)) / fmax_(m1_p, lum_floor) : +inf
//   pixel converged: e_p <= threshold;   tile converged: every such pixel is
//   E_T  = fmax_ over those pixels of e_p, from +0
//   next = n if converged or n >= max_batches, else min(n + step, max_batches)
// fmax_ is minNum/maxNum, which would swallow a NaN moment (the clamp gives var
// 0, the floor the denominator): finite_p keeps such a pixel, and one with an
// infinite moment, from ever counting as converged.  With finite moments e_p is
// finite and >= +0 (the denominator is at least lum_floor > 0), so the all-of
// predicate and the maximum do not depend on the order of the reduction.
struct AdaptiveParams {
  uint32_t min_batches, max_batches, step;
  float threshold, lum_floor;
};
PT_FN bool adaptive_params_ok(uint32_t min_batches, uint32_t max_batches, uint32_t step, float threshold,
                              float lum_floor) {
  const float big = 3.40282347e38f;
  return min_batches >= 2u && max_batches >= min_batches && max_batches <= 65536u && step >= 1u &&
         threshold > 0.0f && threshold <= big && lum_floor > 0.0f && lum_floor <= big;
}
PT_FN float adaptive_error(float m1, float m2, uint32_t n, float lum_floor) {
  const float big = 3.40282347e38f;
  if (!(fabs_(m1) <= big && fabs_(m2) <= big)) return u2f(0x7f800000u);
  return sqrt_(var_of_mean(m1, m2, n)) / fmax_(m1, lum_floor);
}
PT_FN uint32_t adaptive_next(uint32_t n, bool converged, const AdaptiveParams& a) {
  if (converged || n >= a.max_batches) return n;
  return a.max_batches - n < a.step ? a.max_batches : n + a.step;
}
// The rule over a whole W x H image on the host, tiles in raster order (pt_adaptive_select_host; the kernel is
// pt_denoise.hip's adaptive_select_kernel): moments W*H*2 floats, counts, next and errors one per tile; errors
// may be null.
inline void adaptive_select_image(const float* moments, const uint32_t* counts, int W, int H, const AdaptiveParams& a,
                                  uint32_t* next, float* errors) {
  const int bx = (W + 15) / 16, by = (H + 15) / 16;
  for (int ty = 0; ty < by; ++ty)
    for (int tx = 0; tx < bx; ++tx) {
      const int b = ty * bx + tx;
      const uint32_t n = counts[b];
      bool conv = true;
      float e = 0.0f;
      for (int y = ty * 16; y < ty * 16 + 16 && y < H; ++y)
        for (int x = tx * 16; x < tx * 16 + 16 && x < W; ++x) {
          const size_t i = (size_t)y * (size_t)W + (size_t)x;
          const float ep = adaptive_error(moments[2 * i], moments[2 * i + 1], n, a.lum_floor);
          conv = conv && ep <= a.threshold;
          e = fmax_(e, ep);
        }
      next[b] = adaptive_next(n, conv, a);
      if (errors) errors[b] = e;
    }
}

}  // namespace ptdn

namespace ptd {
// The rule per tile (pt_denoise.hip adaptive_select_kernel): next and errors per tile in raster order; added
// (or null) receives next - counts.  counts == next is allowed: a tile's wave reads its count before it writes.
hipError_t launch_adaptive_select(const float2* moments, const uint32_t* counts, int width, int height,
                                  const ptdn::AdaptiveParams& a, uint32_t* next, float* errors, uint32_t* added,
                                  hipStream_t stream);
// The live list of a round from `added` (tiles with added != 0, ascending): entries {x0, y0, first_batch =
// counts - added, n_batches = added}, their number in *n_live.  One workgroup, a scan: the list's order is fixed.
hipError_t launch_adaptive_compact(const uint32_t* counts, const uint32_t* added, int width, int height, int4* list,
                                   int* n_live, hipStream_t stream);
// counts = added = n for every tile (round 0: all tiles render batches 0..n-1).
hipError_t launch_adaptive_fill(uint32_t* counts, uint32_t* added, int n_tiles, uint32_t n, hipStream_t stream);
// var[p] = var_of_mean(m1_p, m2_p, counts[tile of p]).
hipError_t launch_adaptive_var(const float2* moments, const uint32_t* counts, float* var, int width, int height,
                               hipStream_t stream);
// The estimate's launch (pt_denoise.hip spatial_var_kernel): out, distinct from
// the four inputs, receives var where len >= below and the statement elsewhere.
hipError_t launch_spatial_var(const float2* moments, const float* length, const float* variance, const float4* guide,
                              float* out, int width, int height, uint32_t below, int radius, float sn2, float sz2,
                              hipStream_t stream);
}  // namespace ptd
