// pt_denoise.hip — the edge-avoiding a-trous filter's pass kernels
// (pt_denoise), those of the variance-guided filter (pt_denoise_var, below),
// the temporal reprojection kernel (pt_reproject) and the spatial variance
// estimate of short histories (pt_spatial_variance, last); the statements are
// pt_denoise.h, shared with the host.
//
// One pixel per lane, 16x16 pixels per workgroup, a wave a 16x4 strip: the
// lanes of a tile row read 256 consecutive bytes of each image per tap.
// atrous_kernel reads every tap from the images (two 16-B loads per tap, the
// reuse between neighbouring lanes left to the caches); atrous_staged_kernel
// first copies the tile and its halo of 2 * STEP pixels to LDS (steps 1 and 2:
// 20x20 and 24x24 pixels, 12.5 and 18 KB) and taps from there.  Both run
// atrous_pixel over the same values, so their images are the same bits.
#include "pt_denoise.h"
#include "pt_device.h"

#pragma clang fp contract(off)

namespace ptd {
namespace {
using namespace ptdn;

__global__ __launch_bounds__(256) void atrous_kernel(const float4* __restrict__ src, const float4* __restrict__ guide,
                                                     float4* __restrict__ dst, int W, int H, int step, Sigma2 s) {
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const ImageFetch fetch = {src, guide, W};
  dst[(size_t)y * (size_t)W + (size_t)x] = atrous_pixel(fetch, W, H, x, y, step, s);
}

template <int STEP>
struct TileFetch {
  static constexpr int kSide = 16 + 4 * STEP;
  const float4* color;   // LDS, kSide x kSide, pixel (x0 - 2 STEP, y0 - 2 STEP) first
  const float4* guide;
  int x0, y0;            // frame position of the tile's first LDS pixel
  __device__ inline void operator()(int qx, int qy, float4* c, float4* g) const {
    const int i = (qy - y0) * kSide + (qx - x0);
    *c = color[i];
    *g = guide[i];
  }
};

template <int STEP>
__global__ __launch_bounds__(256) void atrous_staged_kernel(const float4* __restrict__ src,
                                                            const float4* __restrict__ guide,
                                                            float4* __restrict__ dst, int W, int H, Sigma2 s) {
  constexpr int kSide = TileFetch<STEP>::kSide;
  __shared__ float4 tc[kSide * kSide], tg[kSide * kSide];
  const int x0 = (int)blockIdx.x * 16 - 2 * STEP, y0 = (int)blockIdx.y * 16 - 2 * STEP;
  for (int i = (int)threadIdx.x; i < kSide * kSide; i += 256) {
    const int gx = x0 + i % kSide, gy = y0 + i / kSide;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {   // atrous_pixel never fetches the others
      const size_t g = (size_t)gy * (size_t)W + (size_t)gx;
      tc[i] = src[g];
      tg[i] = guide[g];
    }
  }
  __syncthreads();
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const TileFetch<STEP> fetch = {tc, tg, x0, y0};
  dst[(size_t)y * (size_t)W + (size_t)x] = atrous_pixel(fetch, W, H, x, y, STEP, s);
}

// ---- the variance-guided filter (pt_denoise_var, pt_denoise.h) --------------
// The same two shapes with a float variance plane beside the colour; the 3x3
// prefilter of the variance is part of the pass (nine 4-B taps around the
// pixel, inside the halo the staged kernel holds anyway).
__global__ __launch_bounds__(256) void moments_var_kernel(const float2* __restrict__ moments, float* __restrict__ var,
                                                          size_t n, uint32_t n_samples) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float2 m = moments[i];
  var[i] = var_of_mean(m.x, m.y, n_samples);
}

__global__ __launch_bounds__(256) void atrous_var_kernel(const float4* __restrict__ src, const float* __restrict__ vsrc,
                                                         const float4* __restrict__ guide, float4* __restrict__ dst,
                                                         float* __restrict__ vdst, int W, int H, int step,
                                                         float sigma_lum, float sn2, float sz2) {
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const VarImageFetch fetch = {src, guide, vsrc, W};
  const VarOut o = atrous_var_pixel(fetch, W, H, x, y, step, sigma_lum, sn2, sz2);
  const size_t i = (size_t)y * (size_t)W + (size_t)x;
  dst[i] = o.c;
  vdst[i] = o.v;
}

template <int STEP>
struct VarTileFetch {
  static constexpr int kSide = 16 + 4 * STEP;
  const float4* color;   // LDS, as TileFetch
  const float4* guide;
  const float* variance;
  int x0, y0;
  __device__ inline void operator()(int qx, int qy, float4* c, float4* g, float* v) const {
    const int i = (qy - y0) * kSide + (qx - x0);
    *c = color[i];
    *g = guide[i];
    *v = variance[i];
  }
  __device__ inline float var(int qx, int qy) const { return variance[(qy - y0) * kSide + (qx - x0)]; }
};

template <int STEP>
__global__ __launch_bounds__(256) void atrous_var_staged_kernel(const float4* __restrict__ src,
                                                                const float* __restrict__ vsrc,
                                                                const float4* __restrict__ guide,
                                                                float4* __restrict__ dst, float* __restrict__ vdst,
                                                                int W, int H, float sigma_lum, float sn2, float sz2) {
  constexpr int kSide = VarTileFetch<STEP>::kSide;
  __shared__ float4 tc[kSide * kSide], tg[kSide * kSide];
  __shared__ float tv[kSide * kSide];
  const int x0 = (int)blockIdx.x * 16 - 2 * STEP, y0 = (int)blockIdx.y * 16 - 2 * STEP;
  for (int i = (int)threadIdx.x; i < kSide * kSide; i += 256) {
    const int gx = x0 + i % kSide, gy = y0 + i / kSide;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {   // atrous_var_pixel never fetches the others
      const size_t g = (size_t)gy * (size_t)W + (size_t)gx;
      tc[i] = src[g];
      tg[i] = guide[g];
      tv[i] = vsrc[g];
    }
  }
  __syncthreads();
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const VarTileFetch<STEP> fetch = {tc, tg, tv, x0, y0};
  const VarOut o = atrous_var_pixel(fetch, W, H, x, y, STEP, sigma_lum, sn2, sz2);
  const size_t i = (size_t)y * (size_t)W + (size_t)x;
  dst[i] = o.c;
  vdst[i] = o.v;
}

// ---- temporal reprojection (pt_reproject, pt_denoise.h reproject_pixel) ------
// The same shape once more: a tile row's lanes read and write consecutive 16-B
// (colour, guide), 8-B (moments) and 4-B (length, variance) words of the
// streamed images.  The four history taps are a gather whose addresses are
// nearly coherent -- neighbouring pixels land on neighbouring history pixels --
// so it is left to the caches; a tap reads its length and guide first and its
// colour and moments only when it is valid.  No LDS.  The camera bases are
// formed on the host (cam_basis) and arrive as kernel arguments.
__global__ __launch_bounds__(256) void reproject_kernel(const float4* __restrict__ color,
                                                        const float2* __restrict__ moments,
                                                        const float4* __restrict__ guide, HistImages hist,
                                                        float4* __restrict__ out_color,
                                                        float2* __restrict__ out_moments,
                                                        float* __restrict__ out_length,
                                                        float* __restrict__ out_variance, CamBasis B, CamBasis Bp,
                                                        int W, int H, float fn, TemporalParams tp) {
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * (size_t)W + (size_t)x;
  const ReprojOut o = reproject_pixel(hist, B, Bp, W, H, x, y, color[i], moments[i], guide[i], fn, tp);
  out_color[i] = o.c;
  out_moments[i] = o.m;
  out_length[i] = o.len;
  out_variance[i] = o.var;
}

// ---- spatial variance of short histories (pt_denoise.h spatial_var_pixel) ----
// The same shape.  Every lane reads its length and variance (a tile row: 64
// consecutive bytes of each); a lane whose history is long enough stores the
// variance and is done.  Only a short lane goes on to its guide and the
// (2r + 1)^2 taps of moments, length and guide (28 B a tap), so a wave with no
// short lane -- and hence a tile with none -- reads neither guide nor moments:
// its branch is skipped on an empty exec mask, no barrier needed.  In a running
// loop a few percent of the first-hit pixels are short, and they come in runs (a
// disoccluded face, a frame edge); the misses stay short for good (they never
// find history), and their taps onto other misses take the statement's
// equal-guide shortcut.  The taps are read from the images: staging a 22x22 halo
// of three images (13.6 KB at r = 3) would make a tile with one short pixel
// read 484 x 28 B to serve 49 taps and cost every tile a barrier; where all
// pixels are short (a first frame) neighbouring lanes' taps overlap and come
// from the caches, as atrous_kernel's do.  That costs 0.0033 ms per tap at
// 1080p, radius 1 to 3 alike, and most of it is the three loads: the shortcut
// takes the exp_ and the divisions off nine pixels in ten of an orbit frame and
// buys 9 %.  A staged variant has not been built; at the default radius 1 it
// could save at most the 0.034 ms the nine taps cost.
__global__ __launch_bounds__(256) void spatial_var_kernel(const float2* __restrict__ moments,
                                                          const float* __restrict__ length,
                                                          const float* __restrict__ variance,
                                                          const float4* __restrict__ guide, float* __restrict__ out,
                                                          int W, int H, float below, int r, float sn2, float sz2) {
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * (size_t)W + (size_t)x;
  const float lenp = length[i];
  float v = variance[i];
  if (lenp < below) {
    const SpatialImageFetch fetch = {moments, length, guide, W};
    v = spatial_var_pixel(fetch, W, H, x, y, r, sn2, sz2, guide[i], lenp);
  }
  out[i] = v;
}

}  // namespace

hipError_t launch_spatial_var(const float2* moments, const float* length, const float* variance, const float4* guide,
                              float* out, int width, int height, uint32_t below, int radius, float sn2, float sz2,
                              hipStream_t stream) {
  if (width <= 0 || height <= 0 || below > 65536u || radius < 1 || radius > kMaxSpatialRadius)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
  spatial_var_kernel<<<grid, 256, 0, stream>>>(moments, length, variance, guide, out, width, height, (float)below,
                                               radius, sn2, sz2);
  return hipGetLastError();
}

hipError_t launch_reproject(const float4* color, const float2* moments, const float4* guide, const float4* hist_color,
                            const float2* hist_moments, const float* hist_length, const float4* hist_guide,
                            float4* out_color, float2* out_moments, float* out_length, float* out_variance,
                            const float cam_cur[16], const float cam_prev[16], int width, int height, uint32_t n,
                            uint32_t max_history, float alpha_min, float normal_min, float depth_rel,
                            hipStream_t stream) {
  if (width <= 0 || height <= 0 || n < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
  const HistImages hist = {hist_color, hist_moments, hist_length, hist_guide};
  const TemporalParams tp = {(float)max_history, alpha_min, normal_min, depth_rel};
  reproject_kernel<<<grid, 256, 0, stream>>>(color, moments, guide, hist, out_color, out_moments, out_length,
                                             out_variance, cam_basis(cam_cur), cam_basis(cam_prev), width, height,
                                             (float)n, tp);
  return hipGetLastError();
}

hipError_t launch_moments_var(const float2* moments, float* var, int width, int height, uint32_t n_samples,
                              hipStream_t stream) {
  if (width <= 0 || height <= 0 || n_samples < 2) return hipErrorInvalidValue;
  const size_t n = (size_t)width * (size_t)height;
  moments_var_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(moments, var, n, n_samples);
  return hipGetLastError();
}

hipError_t launch_atrous_var(const float4* src, const float* vsrc, const float4* guide, float4* dst, float* vdst,
                             int width, int height, int step, float sigma_lum, float sn2, float sz2, bool staged,
                             hipStream_t stream) {
  if (width <= 0 || height <= 0 || step < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
  if (staged && step == 1)
    atrous_var_staged_kernel<1><<<grid, 256, 0, stream>>>(src, vsrc, guide, dst, vdst, width, height, sigma_lum, sn2, sz2);
  else if (staged && step == 2)
    atrous_var_staged_kernel<2><<<grid, 256, 0, stream>>>(src, vsrc, guide, dst, vdst, width, height, sigma_lum, sn2, sz2);
  else
    atrous_var_kernel<<<grid, 256, 0, stream>>>(src, vsrc, guide, dst, vdst, width, height, step, sigma_lum, sn2, sz2);
  return hipGetLastError();
}

hipError_t launch_atrous(const float4* src, const float4* guide, float4* dst, int width, int height, int step,
                         float sc2, float sn2, float sz2, bool staged, hipStream_t stream) {
  if (width <= 0 || height <= 0 || step < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
  const Sigma2 s = {sc2, sn2, sz2};
  if (staged && step == 1)
    atrous_staged_kernel<1><<<grid, 256, 0, stream>>>(src, guide, dst, width, height, s);
  else if (staged && step == 2)
    atrous_staged_kernel<2><<<grid, 256, 0, stream>>>(src, guide, dst, width, height, s);
  else
    atrous_kernel<<<grid, 256, 0, stream>>>(src, guide, dst, width, height, step, s);
  return hipGetLastError();
}

}  // namespace ptd
