// pt_upsample.h — guide-driven upsampling (joint bilateral upsampling, Kopf et
// al., SIGGRAPH 2007): a w x h float4 image rendered at 1/s of the size is put
// onto the W x H = (s*w) x (s*h) grid with the full-size guide image as the
// edge stop.  Stated once for the device kernels (pt_upsample.hip) and the host
// (pt_upsample_host in pt_upsample.cpp), the way pt_denoise.h and pt_display.h
// are: both run these statements, compiled with -ffp-contract=off, so the
// device's bits equal the host's.  Nothing is fused, every division is IEEE.
//
// A pixel's samples are jittered around ndc = 2 * px / W - 1, the pixel's
// lattice point (pt_denoise.h guide_dir), so pixel (i, j) of the w x h frame
// looks along the guide ray of pixel (s*i, s*j) of the full frame: the low
// frame's guide is the full guide at stride s, bit for bit, and one guide, the
// full one G = {n.xyz, t}, serves both ends of a tap.
//
// Every association is fixed here.  For the output pixel (X, Y), s = 2..8:
//   i0 = X / s, j0 = Y / s                                   (integer division)
//   fx = float(X - i0*s) / float(s),  fy likewise            (one IEEE division each)
//   bx[0] = 1 - fx, bx[1] = fx;  by likewise
//   taps (dj outer, di inner) over dj, di in {0, 1}:  i = i0 + di, j = j0 + dj
//      skipped when i >= w or j >= h, and when bx[di] == 0 or by[dj] == 0
//      gq  = G[(j*s) * W + i*s],  gp = G[Y * W + X]
//      d2n = (nx*nx + ny*ny) + nz*nz over gp.xyz - gq.xyz;   dz = gp.w - gq.w
//      wt  = (bx[di] * by[dj]) * exp_(-(d2n / sn2 + (dz*dz) / sz2))
//      sum.rgb += wt * src[j*w + i].rgb;  sum.w += wt         (one add per channel per tap)
//   out.rgb = sum.w > 0 ? sum.rgb / sum.w : src[j0*w + i0].rgb
//   out.a   = src[j0*w + i0].a
// sn2 = sigma_normal * sigma_normal, sz2 = sigma_depth * sigma_depth, both
// finite and non-zero.  The sums start at +0.
//
// A tap of zero bilinear weight is skipped, not multiplied out: 0 * NaN would
// carry a non-finite colour two lattice points away into a pixel on a lattice
// line.  It also gives the lattice identity: at (s*i, s*j) only the tap (i, j)
// is left, its guide is the pixel's own, d2n = dz = 0, the argument is -0,
// exp_(-0) is 1 and out = (0 + 1 * src) / 1: the rendered value (a -0 comes out
// +0).  A hit beside a miss has dz * dz = inf and a weight of 0, as in the
// a-trous tap.  The fallback -- no tap left a weight, or a NaN guide made the
// sum NaN -- is the nearest rendered pixel towards the origin.
#pragma once
#include "pt_display.h"

namespace ptup {
using namespace ptm;

constexpr int kMinScale = 2, kMaxScale = 8;

PT_FN bool params_ok(int scale, float sigma_normal, float sigma_depth) {
  if (scale < kMinScale || scale > kMaxScale) return false;
  const float big = 3.40282347e38f;
  if (!(sigma_normal > 0.0f && sigma_normal <= big && sigma_depth > 0.0f && sigma_depth <= big)) return false;
  const float n2 = sigma_normal * sigma_normal, z2 = sigma_depth * sigma_depth;
  return n2 > 0.0f && n2 <= big && z2 > 0.0f && z2 <= big;
}

// The frame sizes the index arithmetic holds: W * H full-size pixels at most 2^31.
PT_FN bool size_ok(int w, int h, int s) {
  return w > 0 && h > 0 && (long long)w * s * ((long long)h * s) <= (1ll << 31);
}

// What a pixel needs beside the images: the low size, the scale and the squared sigmas.
struct Frame {
  int w, h, s;
  float sn2, sz2;
};

// One output pixel.  src is the w x h colour, guide the (s*w) x (s*h) guide.
PT_FN float4 upsample_pixel(const float4* src, const float4* guide, const Frame& f, int X, int Y) {
  const int s = f.s;
  const size_t W = (size_t)f.w * (size_t)s;
  const int i0 = X / s, j0 = Y / s;
  const float fx = (float)(X - i0 * s) / (float)s;
  const float fy = (float)(Y - j0 * s) / (float)s;
  const float4 gp = guide[(size_t)Y * W + (size_t)X];
  float4 sum;
  sum.x = sum.y = sum.z = sum.w = 0.0f;
  for (int dj = 0; dj < 2; ++dj) {
    const int j = j0 + dj;
    const float by = dj ? fy : 1.0f - fy;
    if (j >= f.h || by == 0.0f) continue;
    for (int di = 0; di < 2; ++di) {
      const int i = i0 + di;
      const float bx = di ? fx : 1.0f - fx;
      if (i >= f.w || bx == 0.0f) continue;
      const float4 gq = guide[((size_t)j * (size_t)s) * W + (size_t)i * (size_t)s];
      const float4 cq = src[(size_t)j * (size_t)f.w + (size_t)i];
      const float nx = gp.x - gq.x, ny = gp.y - gq.y, nz = gp.z - gq.z;
      const float d2n = (nx * nx + ny * ny) + nz * nz;
      const float dz = gp.w - gq.w;
      const float wt = (bx * by) * exp_(-(d2n / f.sn2 + (dz * dz) / f.sz2));
      sum.x += wt * cq.x;
      sum.y += wt * cq.y;
      sum.z += wt * cq.z;
      sum.w += wt;
    }
  }
  const float4 c0 = src[(size_t)j0 * (size_t)f.w + (size_t)i0];
  float4 out = c0;
  if (sum.w > 0.0f) {
    out.x = sum.x / sum.w;
    out.y = sum.y / sum.w;
    out.z = sum.z / sum.w;
  }
  return out;
}

}  // namespace ptup

namespace ptd {
// pt_upsample.hip.  src is w x h, guide and dst are (scale*w) x (scale*h), all in row order and
// distinct.  launch_upsample writes float4 pixels; launch_upsample_display runs the same statement
// and pt_display.h's on its result, and writes one RGBA8 word a pixel (state as launch_display's).
hipError_t launch_upsample(const float4* src, const float4* guide, float4* dst, int w, int h, int scale, float sn2,
                           float sz2, hipStream_t stream);
hipError_t launch_upsample_display(const float4* src, const float4* guide, uint32_t* dst, int w, int h, int scale,
                                   float sn2, float sz2, int tonemap, float exposure, float w2,
                                   const ptdp::MeterState* state, hipStream_t stream);
}  // namespace ptd
