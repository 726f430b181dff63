// pt_denoise.hip — the edge-avoiding a-trous filter's pass kernels
// (pt_denoise), those of the variance-guided filter (pt_denoise_var, below),
// the temporal reprojection kernel (pt_reproject), the spatial variance
// estimate of short histories (pt_spatial_variance) and the adaptive stopping
// rule with its live list and variance plane (pt_adaptive_select,
// pt_adaptive_advance, pt_adaptive_denoise; last); the statements are
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

// ---- adaptive sampling: the stopping rule per tile (pt_denoise.h adaptive_error) ----
// One wave per 16x16 tile, four tiles per workgroup.  Lane l takes the pixels
// (l & 15, (l >> 4) + 4k), k = 0..3: per k the wave reads four tile rows, 128
// consecutive bytes of moments each.  A pixel outside the frame is not read and
// counts as converged with e = +0 by a select, not a branch, so every lane of
// the wave reaches the ballot and the shuffles; only whole waves past the last
// tile leave, on a wave-uniform test.  The predicate is reduced by a ballot, the
// error by a butterfly of maxima (order-free: e is never NaN); lane 0 writes.
__global__ __launch_bounds__(256) void adaptive_select_kernel(const float2* __restrict__ moments,
                                                              const uint32_t* __restrict__ counts, int W, int H,
                                                              int blocks_x, int n_tiles, AdaptiveParams a,
                                                              uint32_t* __restrict__ next, float* __restrict__ errors,
                                                              uint32_t* __restrict__ added) {
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  const int b = (int)blockIdx.x * 4 + wave;
  if (b >= n_tiles) return;   // wave-uniform
  const uint32_t n = counts[b];
  const int x = (b % blocks_x) * 16 + (lane & 15);
  const int y0 = (b / blocks_x) * 16 + (lane >> 4);
  bool conv = true;
  float e = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + 4 * k;
    const bool in = x < W && y < H;
    float2 m = make_float2(0.0f, 0.0f);
    if (in) m = moments[(size_t)y * (size_t)W + (size_t)x];
    const float ep = adaptive_error(m.x, m.y, n, a.lum_floor);   // of +0 moments: +0
    conv = conv && (!in || ep <= a.threshold);
    e = fmax_(e, in ? ep : 0.0f);
  }
  const bool tile_conv = __builtin_amdgcn_ballot_w64(!conv) == 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) e = fmax_(e, __shfl_xor(e, off, 64));
  if (lane == 0) {
    const uint32_t nx = adaptive_next(n, tile_conv, a);
    next[b] = nx;
    errors[b] = e;
    if (added) added[b] = nx - n;
  }
}

// The live list: thread t takes the tiles [t * per, (t + 1) * per), counts its live ones, the
// workgroup scans the 256 counts (a wave's by shuffles, the four waves' totals through LDS), and
// each thread writes its entries from its offset on -- ascending tile order, no atomics.
__global__ __launch_bounds__(256) void adaptive_compact_kernel(const uint32_t* __restrict__ counts,
                                                               const uint32_t* __restrict__ added, int blocks_x,
                                                               int n_tiles, int4* __restrict__ list,
                                                               int* __restrict__ n_live) {
  __shared__ int wave_total[4];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int per = (n_tiles + 255) / 256;
  const int lo = min(t * per, n_tiles), hi = min(lo + per, n_tiles);
  int mine = 0;
  for (int b = lo; b < hi; ++b) mine += added[b] != 0u ? 1 : 0;
  int incl = mine;   // inclusive scan within the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  if (lane == 63) wave_total[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wave_total[w];
  int pos = base + incl - mine;
  for (int b = lo; b < hi; ++b) {
    const uint32_t ad = added[b];
    if (ad == 0u) continue;
    list[pos++] = make_int4((b % blocks_x) * 16, (b / blocks_x) * 16, (int)(counts[b] - ad), (int)ad);
  }
  if (t == 255) *n_live = base + incl;
}

__global__ __launch_bounds__(256) void adaptive_fill_kernel(uint32_t* __restrict__ counts, uint32_t* __restrict__ added,
                                                            int n_tiles, uint32_t n) {
  const int b = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (b >= n_tiles) return;
  counts[b] = n;
  added[b] = n;
}

// The variance plane of an adaptive render: the variance of the mean at each tile's own count.
__global__ __launch_bounds__(256) void adaptive_var_kernel(const float2* __restrict__ moments,
                                                           const uint32_t* __restrict__ counts,
                                                           float* __restrict__ var, int W, int H) {
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  if (x >= W || y >= H) return;
  const size_t i = (size_t)y * (size_t)W + (size_t)x;
  const float2 m = moments[i];
  var[i] = var_of_mean(m.x, m.y, counts[blockIdx.y * gridDim.x + blockIdx.x]);
}

}  // namespace

hipError_t launch_adaptive_select(const float2* moments, const uint32_t* counts, int width, int height,
                                  const AdaptiveParams& a, uint32_t* next, float* errors, uint32_t* added,
                                  hipStream_t stream) {
  if (width <= 0 || height <= 0) return hipErrorInvalidValue;
  const int bx = (width + 15) / 16, n_tiles = bx * ((height + 15) / 16);
  adaptive_select_kernel<<<(unsigned)((n_tiles + 3) / 4), 256, 0, stream>>>(moments, counts, width, height, bx, n_tiles,
                                                                           a, next, errors, added);
  return hipGetLastError();
}

hipError_t launch_adaptive_compact(const uint32_t* counts, const uint32_t* added, int width, int height, int4* list,
                                   int* n_live, hipStream_t stream) {
  if (width <= 0 || height <= 0) return hipErrorInvalidValue;
  const int bx = (width + 15) / 16, n_tiles = bx * ((height + 15) / 16);
  adaptive_compact_kernel<<<1, 256, 0, stream>>>(counts, added, bx, n_tiles, list, n_live);
  return hipGetLastError();
}

hipError_t launch_adaptive_fill(uint32_t* counts, uint32_t* added, int n_tiles, uint32_t n, hipStream_t stream) {
  if (n_tiles <= 0) return hipErrorInvalidValue;
  adaptive_fill_kernel<<<(unsigned)((n_tiles + 255) / 256), 256, 0, stream>>>(counts, added, n_tiles, n);
  return hipGetLastError();
}

hipError_t launch_adaptive_var(const float2* moments, const uint32_t* counts, float* var, int width, int height,
                               hipStream_t stream) {
  if (width <= 0 || height <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
  adaptive_var_kernel<<<grid, 256, 0, stream>>>(moments, counts, var, width, height);
  return hipGetLastError();
}

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
