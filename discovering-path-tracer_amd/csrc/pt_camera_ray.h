// pt_camera_ray.h — main()'s ray generation (raytrace_comp.comp:430-460) for one
// pixel and one sample batch: the aperture draw, the jitter draw, the focal
// point.  One statement for the wavefront pipeline's PH_BEGIN (kernels/wf_state.h
// path_step), pt_camera_rays' kernel (kernels/radiance.h) and its host
// statement (pt_radiance_host.cpp); render_kernel states the same operations
// itself, hoisted around its sample loop.  pt_math.h's forms, -ffp-contract=off.
#pragma once
#include "pt_math.h"

namespace ptd {
using namespace ptm;

struct CamFrame {
  v3 cpos, cdir, right, up;
  float tanFov, aspect, ndcX0, ndcY0;
  int W, H, px, py;
};

// The frame of pixel (px, py) of a W x H image: the camera's position, direction and the right / up
// vectors main() derives (pt_denoise.h cam_basis), with tan(radians(fov / 2)).
__host__ __device__ static __forceinline__ CamFrame cam_frame(v3 cpos, v3 cdir, v3 right, v3 up, float tan_fov, int W,
                                                              int H, int px, int py) {
  CamFrame F;
  F.cpos = cpos;
  F.cdir = cdir;
  F.right = right;
  F.up = up;
  F.W = W;
  F.H = H;
  F.px = px;
  F.py = py;
  F.ndcX0 = (2.0f * (float)px / (float)W) - 1.0f;
  F.ndcY0 = (2.0f * (float)py / (float)H) - 1.0f;
  F.aspect = (float)W / (float)H;
  F.tanFov = tan_fov;
  return F;
}

// main() ray generation (:430-460) for one sample batch.
__host__ __device__ static __forceinline__ void camera_ray(const CamFrame& F, uint32_t seed, v3* origin, v3* dir) {
  uint32_t rng = seed;
  float u1 = fmax_(1e-38f, rng_next(&rng));
  float u2 = rng_next(&rng);
  float r = sqrt_(-2.0f * log_(u1));
  float th = (2.0f * 0x1.921fb6p+1f) * u2;
  float sn, cs;
  sincos_(th, &sn, &cs);
  const float ax = (r * cs) * 0.02f;
  const float ay = (r * sn) * 0.02f;
  *origin = add(add(F.cpos, muls(F.right, ax)), muls(F.up, ay));
  u1 = fmax_(1e-38f, rng_next(&rng));
  u2 = rng_next(&rng);
  r = sqrt_(-2.0f * log_(u1));
  th = (2.0f * 0x1.921fb6p+1f) * u2;
  sincos_(th, &sn, &cs);
  const float jx = r * cs, jy = r * sn;
  const float ndcX = F.ndcX0 + (jx * 0.5f) / (float)F.W;
  const float ndcY = F.ndcY0 + (jy * 0.5f) / (float)F.H;
  const v3 bdir =
      normalize(sub(add(F.cdir, muls(neg(F.right), (ndcX * F.tanFov) * F.aspect)), muls(F.up, ndcY * F.tanFov)));
  const v3 focal = add(F.cpos, muls(bdir, 3.0f));
  *dir = normalize(sub(focal, *origin));
}

// The seed of pixel (px, py)'s sample of batch `batch` (:436-438), uint32 wrap-around: pt_ray::reserved of
// pt_camera_rays.
__host__ __device__ static __forceinline__ uint32_t camera_seed(uint32_t batch, int W, int H, int px, int py) {
  return (batch * (uint32_t)H + (uint32_t)py) * (uint32_t)W + (uint32_t)px;
}

}  // namespace ptd
