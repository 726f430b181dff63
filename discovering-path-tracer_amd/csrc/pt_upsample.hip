// pt_upsample.hip — the kernels of guide-driven upsampling (pt_upsample,
// pt_upsample_display); the statement is pt_upsample.h, shared with the host.
//
// Both kernels take one output pixel a lane, 16x16 pixels a workgroup, a wave a
// 16x4 strip as in the filters: a wave reads four 256-B runs of the guide and
// writes four 256-B runs of float4 (upsample_kernel) or four 64-B runs of RGBA8
// words (upsample_display_kernel).  A workgroup's tile touches (16/s + 1)^2
// lattice points of colour and guide, 81 at s = 2; the lanes tap them from
// global memory.  Neighbouring lanes share their lattice points (at s = 2 a
// wave's 64 lanes read 27 distinct ones), so a tap's load is served by a few
// cache lines that the same workgroup has just touched, and the only traffic
// that reaches memory is the floor: the guide once, the source once, the
// result once.  Staging the 81 taps in LDS would save none of it and costs a
// barrier; profiles/upsample/ holds the times against that floor.
//
// upsample_display_kernel runs pt_display.h's pixel on the upsampled value
// without storing it: the full-size float image is neither written nor read
// back, 32 B a pixel less than pt_upsample followed by pt_display.  It copies
// the threshold table to LDS first, as display_kernel does.
#include "pt_upsample.h"

#pragma clang fp contract(off)

namespace ptd {
namespace {
using namespace ptup;

__global__ __launch_bounds__(256) void upsample_kernel(const float4* __restrict__ src,
                                                       const float4* __restrict__ guide, float4* __restrict__ dst,
                                                       Frame f) {
  const int X = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int Y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  const int W = f.w * f.s, H = f.h * f.s;
  if (X >= W || Y >= H) return;
  dst[(size_t)Y * (size_t)W + (size_t)X] = upsample_pixel(src, guide, f, X, Y);
}

__global__ __launch_bounds__(256) void upsample_display_kernel(const float4* __restrict__ src,
                                                               const float4* __restrict__ guide,
                                                               uint32_t* __restrict__ dst, Frame f, ptdp::Tone t,
                                                               const ptdp::MeterState* __restrict__ state) {
  __shared__ uint32_t T[256];
  T[threadIdx.x] = ptdp::kSrgb8T[threadIdx.x];
  __syncthreads();
  if (state) t.scale = t.scale * state->scale;   // exposure * auto_scale
  const int X = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int Y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  const int W = f.w * f.s, H = f.h * f.s;
  if (X >= W || Y >= H) return;
  dst[(size_t)Y * (size_t)W + (size_t)X] = ptdp::display_pixel(T, upsample_pixel(src, guide, f, X, Y), t);
}

bool launch_ok(int w, int h, int scale, dim3* grid) {
  if (scale < kMinScale || scale > kMaxScale || !size_ok(w, h, scale)) return false;
  const long long by = ((long long)h * scale + 15) / 16;
  if (by > 65535) return false;   // the grid's y extent
  *grid = dim3((unsigned)(((long long)w * scale + 15) / 16), (unsigned)by);
  return true;
}

}  // namespace

hipError_t launch_upsample(const float4* src, const float4* guide, float4* dst, int w, int h, int scale, float sn2,
                           float sz2, hipStream_t stream) {
  dim3 grid;
  if (!launch_ok(w, h, scale, &grid)) return hipErrorInvalidValue;
  const Frame f = {w, h, scale, sn2, sz2};
  upsample_kernel<<<grid, 256, 0, stream>>>(src, guide, dst, f);
  return hipGetLastError();
}

hipError_t launch_upsample_display(const float4* src, const float4* guide, uint32_t* dst, int w, int h, int scale,
                                   float sn2, float sz2, int tonemap, float exposure, float w2,
                                   const ptdp::MeterState* state, hipStream_t stream) {
  dim3 grid;
  if (!launch_ok(w, h, scale, &grid)) return hipErrorInvalidValue;
  const Frame f = {w, h, scale, sn2, sz2};
  const ptdp::Tone t = {tonemap, exposure, w2};
  upsample_display_kernel<<<grid, 256, 0, stream>>>(src, guide, dst, f, t, state);
  return hipGetLastError();
}

}  // namespace ptd
