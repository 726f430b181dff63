// pt_rays_host.h — the host statement of the batched ray queries
// (pt_trace_rays_host): the reference's traceRay (raytrace_comp.comp:159-204)
// and occluded() statement (:359, :398) over the reference's own node array.
// Host only: no HIP runtime call, no context, nothing from the oracle; a
// stand-alone program builds it with scene/threaded_bvh.cpp
// (tests/rays_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "pt_isect.h"

namespace ptr {

// The scene as the walk reads it, and the walk itself: shared with the host statement of the radiance
// queries (pt_radiance_host.cpp), whose every ray is this traceRay.
struct Scene {
  const float* nodes;
  std::vector<int32_t> left, right;   // the links, decoded once
  std::vector<float4> tris;           // by triangle index: {v0, e1.x} {e1.yz, e2.xy} {e2.z, n} (pt_device.h)
};
// "" or why the arrays are not a scene (what pt_upload_scene refuses).  *out keeps `nodes`.
std::string make_scene(const float* vertices, size_t n_vertex_floats, const uint32_t* indices, size_t n_indices,
                       const float* nodes, size_t n_nodes, bool int_bits, Scene* out);
// limit null: the closest hit into *best / *bt (1e30f / -1: none), returns false; else whether the ray is
// occluded below *limit.  stack: scratch the caller keeps across rays.
bool walk(const Scene& s, ptm::v3 o, ptm::v3 d, const float* limit, std::vector<int32_t>& stack, float* best,
          int32_t* bt);

// rays: n x 8 floats {o, d, limit, -}.  kind 0: out = n x 8 words {t, tri, u, v, n.xyz, 0}; kind 1: out = n
// words, 1 occluded.  nodes: 8 floats each, links float- or int-encoded.  threads <= 0: one per core.
// Returns "" or why the arrays are not a scene (what pt_upload_scene refuses).
std::string trace_rays_host(const float* vertices, size_t n_vertex_floats, const uint32_t* indices, size_t n_indices,
                            const float* nodes, size_t n_nodes, bool int_bits, int kind, const float* rays, size_t n,
                            void* out, int threads);

}  // namespace ptr
