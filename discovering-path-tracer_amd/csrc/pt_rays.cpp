// pt_rays.cpp — batched ray queries behind the C ABI (include/pathtracer.h):
// pt_trace_rays on device memory, pt_trace_rays_sync through library-owned
// staging buffers, and pt_trace_rays_host, the host statement
// (pt_rays_host.cpp).  The kernels are csrc/kernels/rays.h.
#include <stdint.h>

#include <algorithm>
#include <string>

#include "pt_context.h"
#include "pt_plan.h"
#include "pt_rays_host.h"

static_assert(sizeof(pt_ray) == 32 && sizeof(pt_hit) == 32, "pt_ray and pt_hit are two float4 each (kernels/rays.h)");
static_assert(PT_RAYS_CLOSEST == ptd::kRaysClosest && PT_RAYS_ANY == ptd::kRaysAny, "the kinds of pt_device.h");

// Frees what this file allocates in a context (pt_destroy).
void rays_release(pt_context* c) {
  dev_free(c->d_rays_counters);
  dev_free(c->d_rays_slot);
  dev_free(c->d_rays_in);
  dev_free(c->d_rays_out);
  c->rays_slot_cap = c->rays_in_cap = c->rays_out_cap = 0;
  c->rays_slot_serial = -1;
}

// What every entry point checks first.  n == 0 passes (the callers then do nothing).
static int rays_args(const pt_context* c, int kind, const void* rays, size_t n, const void* out) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (kind != PT_RAYS_CLOSEST && kind != PT_RAYS_ANY) return fail(PT_ERR_INVALID, "kind is PT_RAYS_CLOSEST or PT_RAYS_ANY");
  if (n > (size_t)ptd::kRaysMax) return fail(PT_ERR_INVALID, "more than 2^31 - 256 rays in one call");
  if (n > 0 && (!rays || !out)) return fail(PT_ERR_INVALID, "null argument");
  return PT_OK;
}

// What the wide kernel needs beside wide_params' arrays: its two counters, and the rank -> triangle
// index table of the scene's wide tree, built on the device by the first query after an upload.
static int rays_wide_state(pt_context* c) {
  if (!c->d_rays_counters) PT_HIP(hipMalloc((void**)&c->d_rays_counters, 2 * sizeof(uint32_t)));
  if (c->rays_slot_serial == c->scene_serial && c->d_rays_slot) return PT_OK;
  const int rg = grow_dev(c, &c->d_rays_slot, &c->rays_slot_cap, (size_t)c->n_tris);
  if (rg) return rg;
  PT_HIP(ptd::launch_rays_slots(c->d_wide_rank_of, c->n_tris, c->d_rays_slot, c->stream));
  c->rays_slot_serial = c->scene_serial;
  return PT_OK;
}

extern "C" {

int pt_trace_rays(pt_context* c, int kind, const void* d_rays, size_t n, void* d_out) {
  PT_SINGLE(c, "pt_trace_rays");
  const int ra = rays_args(c, kind, d_rays, n, d_out);
  if (ra) return ra;
  if (n == 0) return PT_OK;
  if (((uintptr_t)d_rays | (uintptr_t)d_out) & 15u) return fail(PT_ERR_INVALID, "device pointers must be 16-B aligned");
  PT_HIP(hipSetDevice(c->device));
  // the scene's share of frame_params: a query needs no frame and no camera
  ptd::RenderParams p{};
  p.nodes = c->d_nodes;
  p.n_nodes = c->n_nodes;
  p.tris = c->d_tris;
  p.hit_tris = c->d_tris;
  p.n_tris = c->n_tris;
  p.n_cull = -1;
  p.wf_grid = c->opt_wf_grid;
  p.wide_refill = c->opt_wf_refill > 0 ? c->opt_wf_refill : (c->opt_wf_grid < 100 ? 8 : 16);   // plan_launch's auto
  // the wide walk first, then the LDS rule (pt_plan.h), as pt_render_guide
  const bool wide = c->opt_wide && c->n_wide > 0;
  const bool fits = lds_fits(*c, c->n_nodes);
  if (!wide && lds_refused(*c, fits)) return fail(PT_ERR_UNSUPPORTED, kLdsTooLarge);
  const bool lds = !wide && lds_staged(*c, fits);
  const int ro = order_shared(c);   // the overflow areas and the counters are the context's
  if (ro) return ro;
  if (wide) {
    const int rw = wide_params(c, &p);
    if (rw) return rw;
    p.wide_handback = c->opt_wide == 2 ? 1 : 0;
    const int rs = rays_wide_state(c);
    if (rs) return rs;
  }
  PT_HIP(ptd::launch_rays(p, kind, d_rays, n, d_out, c->d_rays_counters, c->d_rays_slot, lds, c->opt_rays_refill != 0,
                          c->stream));
  return mark_shared(c);
}

int pt_trace_rays_sync(pt_context* c, int kind, const pt_ray* rays, size_t n, void* out) {
  PT_SINGLE(c, "pt_trace_rays_sync");
  const int ra = rays_args(c, kind, rays, n, out);
  if (ra) return ra;
  if (n == 0) return PT_OK;
  PT_HIP(hipSetDevice(c->device));
  // in chunks, so that the staging buffers stay small beside a large batch
  const size_t chunk = std::min<size_t>(n, (size_t)1 << 22);
  const size_t out_bytes = kind == PT_RAYS_ANY ? sizeof(uint32_t) : sizeof(pt_hit);
  typedef struct { char b[32]; } Rec;
  Rec *in = (Rec*)c->d_rays_in, *ob = (Rec*)c->d_rays_out;
  int rg = grow_dev(c, &in, &c->rays_in_cap, chunk);
  c->d_rays_in = in;
  if (rg) return rg;
  rg = grow_dev(c, &ob, &c->rays_out_cap, chunk);
  c->d_rays_out = ob;
  if (rg) return rg;
  for (size_t i0 = 0; i0 < n; i0 += chunk) {
    const size_t m = std::min(chunk, n - i0);
    PT_HIP(hipMemcpyAsync(c->d_rays_in, rays + i0, m * sizeof(pt_ray), hipMemcpyHostToDevice, c->stream));
    const int rt = pt_trace_rays(c, kind, c->d_rays_in, m, c->d_rays_out);
    if (rt) return rt;
    PT_HIP(hipMemcpyAsync((char*)out + i0 * out_bytes, c->d_rays_out, m * out_bytes, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
  }
  return PT_OK;
}

int pt_trace_rays_host(const float* vertices, size_t n_vertex_floats, const uint32_t* indices, size_t n_indices,
                       const pt_bvh_node* nodes, size_t n_nodes, uint32_t flags, int kind, const pt_ray* rays, size_t n,
                       void* out, int threads) {
  if (!vertices || !indices || !nodes) return fail(PT_ERR_INVALID, "null scene array");
  if (kind != PT_RAYS_CLOSEST && kind != PT_RAYS_ANY) return fail(PT_ERR_INVALID, "kind is PT_RAYS_CLOSEST or PT_RAYS_ANY");
  if (n > 0 && (!rays || !out)) return fail(PT_ERR_INVALID, "null argument");
  const std::string why =
      ptr::trace_rays_host(vertices, n_vertex_floats, indices, n_indices, (const float*)nodes, n_nodes,
                           (flags & PT_NODES_INT_BITS) != 0, kind, (const float*)rays, n, out, threads);
  if (!why.empty()) return fail(PT_ERR_SCENE, why);
  return PT_OK;
}

}  // extern "C"
