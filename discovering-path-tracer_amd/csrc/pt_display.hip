// pt_display.hip — the display transform's kernels (pt_display): the per-pixel
// exposure, tone map and sRGB encode, and the two metering stages behind auto
// exposure; the statements are pt_display.h, shared with the host.
//
// display_kernel treats the image as n = W * H pixels in a row (the transform is
// pointwise), one pixel a lane: a wave reads 1 KB of consecutive float4 and
// writes 256 consecutive bytes.  Every workgroup first copies the 1-KB threshold
// table to LDS (one entry a lane), where the eight compare steps of a channel
// read it at per-lane addresses.  A shape of four pixels a lane (64 B read, one
// 16-B store, the ragged end word by word) was built and measured 8-13 % slower
// for every operator (profiles/display/timing_1080p.json): its loads are 64 B
// apart between neighbouring lanes, four half-used lines a load where this shape
// reads whole ones, and the wider store buys nothing at 4 B a pixel.
//
// display_meter_kernel is stage one of the metering, one workgroup per 16x16
// tile, display_meter_finish_kernel stage two, one workgroup: the 256 terms sit
// in LDS and every step of tree256 runs its lanes side by side, a barrier
// between steps.  The count goes through a ballot per wave and is exact in any
// order.  The finish writes the scale to device memory, where display_kernel
// reads it: the host never waits for it.
#include "pt_display.h"

#pragma clang fp contract(off)

namespace ptd {
namespace {
using namespace ptdp;

__global__ __launch_bounds__(256) void display_kernel(const float4* __restrict__ src, uint32_t* __restrict__ dst,
                                                      size_t n, Tone t, const MeterState* __restrict__ state) {
  __shared__ uint32_t T[256];
  T[threadIdx.x] = kSrgb8T[threadIdx.x];
  __syncthreads();
  if (state) t.scale = t.scale * state->scale;   // exposure * auto_scale
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dst[i] = display_pixel(T, src[i], t);
}

// The sum of the 256 lane values by tree256 and of the lanes' counts; the results are lane 0's.
__device__ inline void block_reduce(float* v, uint32_t* wave_n, float term, bool counted, float* sum, uint32_t* n) {
  const int i = (int)threadIdx.x;
  v[i] = term;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(counted);
  if ((i & 63) == 0) wave_n[i >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (i < s) tree_step(v, i, s);
    __syncthreads();
  }
  *sum = v[0];
  *n = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

__global__ __launch_bounds__(256) void display_meter_kernel(const float4* __restrict__ src, int W, int H,
                                                            float* __restrict__ partial_sum,
                                                            uint32_t* __restrict__ partial_n) {
  __shared__ float v[256];
  __shared__ uint32_t wave_n[4];
  const int x = (int)blockIdx.x * 16 + ((int)threadIdx.x & 15);
  const int y = (int)blockIdx.y * 16 + ((int)threadIdx.x >> 4);
  float term = 0.0f;
  bool metered = false;
  if (x < W && y < H) term = meter_term(src[(size_t)y * (size_t)W + (size_t)x], &metered);
  float sum;
  uint32_t n;
  block_reduce(v, wave_n, term, metered, &sum, &n);
  if (threadIdx.x == 0) {
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partial_sum[tile] = sum;
    partial_n[tile] = n;
  }
}

__global__ __launch_bounds__(256) void display_meter_finish_kernel(const float* __restrict__ partial_sum,
                                                                   const uint32_t* __restrict__ partial_n,
                                                                   int n_tiles, float key, float adapt, int have_prev,
                                                                   MeterState* __restrict__ state) {
  __shared__ float v[256];
  __shared__ uint32_t cnt[256];
  const int j = (int)threadIdx.x;
  uint32_t mine = 0u;
#pragma unroll 8
  for (int t = j; t < n_tiles; t += 256) mine += partial_n[t];
  v[j] = meter_lane(partial_sum, n_tiles, j);
  cnt[j] = mine;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (j < s) {
      tree_step(v, j, s);
      cnt[j] += cnt[j + s];
    }
    __syncthreads();
  }
  if (j == 0) {
    const uint32_t n = cnt[0];
    state->scale = meter_scale(v[0], n, key, adapt, have_prev != 0, have_prev ? state->scale : 1.0f);
    state->n = n;
  }
}

}  // namespace

hipError_t launch_display(const float4* src, uint32_t* dst, size_t n_pixels, int tonemap, float exposure, float w2,
                          const MeterState* state, hipStream_t stream) {
  if (n_pixels == 0 || n_pixels > ((size_t)1 << 31)) return hipErrorInvalidValue;
  const Tone t = {tonemap, exposure, w2};
  display_kernel<<<(unsigned)((n_pixels + 255) / 256), 256, 0, stream>>>(src, dst, n_pixels, t, state);
  return hipGetLastError();
}

hipError_t launch_display_meter(const float4* src, int width, int height, float* partial_sum, uint32_t* partial_n,
                                float key, float adapt, int have_prev, MeterState* state, hipStream_t stream) {
  if (width <= 0 || height <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
  display_meter_kernel<<<grid, 256, 0, stream>>>(src, width, height, partial_sum, partial_n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  display_meter_finish_kernel<<<1, 256, 0, stream>>>(partial_sum, partial_n, (int)(grid.x * grid.y), key, adapt,
                                                     have_prev, state);
  return hipGetLastError();
}

}  // namespace ptd
