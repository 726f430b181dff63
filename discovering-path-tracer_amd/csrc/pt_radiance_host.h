// pt_radiance_host.h — the host statement of the radiance queries
// (pt_trace_radiance_host) and of the camera's own rays (pt_camera_rays_host):
// the shader's pathTrace (raytrace_comp.comp:300-418) along the caller's ray
// from the caller's seed, its running mean (:467-469) over the query's samples,
// and main()'s ray generation (:430-460).  Host only: no HIP runtime call, no
// context, nothing from the oracle; every ray is pt_rays_host.h's walk.  A
// stand-alone program builds it with pt_rays_host.cpp and the scene layer
// (tests/radiance_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

namespace ptr {

// One light as pt_upload_lights takes it: position, normal, intensity, size, 4 floats each (pt_area_light).
// rays: n x 8 words {o, d, -, seed}; out: n x 4 floats.  Sample s of query q is
// pathTrace(o, d, seed + s * seed_stride) in uint32 arithmetic; the n_samples colours are folded in order
// from {+0, +0, +0, +0} by (acc * float(s) + c) / float(s + 1), alpha folding 1.  threads <= 0: one per core.
// Returns "" or why the arrays are not a scene.
std::string trace_radiance_host(const float* vertices, size_t n_vertex_floats, const uint32_t* indices,
                                size_t n_indices, const float* nodes, size_t n_nodes, bool int_bits,
                                const float* lights, size_t n_lights, int max_depth, int sss_bounces,
                                uint32_t n_samples, uint32_t seed_stride, const float* rays, size_t n, float* out,
                                int threads);

// main()'s ray of pixel pixels[i] = y * W + x (null: pixel i) for sample batch `batch` of the camera block
// cam[16] (pos@0, dir@4, up@8, fov@12): rays[i] = {origin, dir, 1e30f, (batch * H + y) * W + x}.
void camera_rays_host(const float cam[16], int W, int H, uint32_t batch, const int32_t* pixels, size_t n, float* rays);

}  // namespace ptr
