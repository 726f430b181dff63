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

namespace ptr {

// rays: n x 8 floats {o, d, limit, -}.  kind 0: out = n x 8 words {t, tri, u, v, n.xyz, 0}; kind 1: out = n
// words, 1 occluded.  nodes: 8 floats each, links float- or int-encoded.  threads <= 0: one per core.
// Returns "" or why the arrays are not a scene (what pt_upload_scene refuses).
std::string trace_rays_host(const float* vertices, size_t n_vertex_floats, const uint32_t* indices, size_t n_indices,
                            const float* nodes, size_t n_nodes, bool int_bits, int kind, const float* rays, size_t n,
                            void* out, int threads);

}  // namespace ptr
