// pt_radiance.cpp — radiance queries behind the C ABI (include/pathtracer.h):
// pt_trace_radiance on device memory, pt_trace_radiance_sync through
// library-owned staging buffers, pt_camera_rays, and the two host statements
// (pt_radiance_host.cpp).  The kernels are csrc/kernels/radiance.h; which of
// them a call runs is plan_launch's answer for a launch of as many paths.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "pt_context.h"
#include "pt_plan.h"
#include "pt_radiance_host.h"

static_assert(sizeof(pt_ray) == 32, "a query is two float4 (kernels/radiance.h)");
static_assert(sizeof(pt_area_light) == 64, "a light is 16 floats (pt_radiance_host.h)");

// Paths of a chunk under PT_OPT_RADIANCE_CHUNK 0: the rays of a 1080p frame in one chunk; 64 MiB of colours
// on the path-recursive kernel, 1.7 GB of path state (ptd::kWfBytesPerPath = 416 B) on the wavefront pipeline.
constexpr long long kRadianceAutoChunk = 1ll << 22;

// Frees what this file allocates in a context (pt_destroy).
void radiance_release(pt_context* c) {
  dev_free(c->d_rad_colors);
  dev_free(c->d_rad_in);
  dev_free(c->d_rad_out);
  c->rad_colors_cap = c->rad_in_cap = c->rad_out_cap = 0;
}

static int radiance_params(const pt_radiance_params* in, pt_radiance_params* p) {
  if (in)
    *p = *in;
  else
    (void)pt_radiance_default_params(p);
  if (p->n_samples < 1u || p->n_samples > ptd::kRadianceMaxSamples)
    return fail(PT_ERR_INVALID, "pt_radiance_params: 1 <= n_samples <= 65536");
  return PT_OK;
}

// What every entry point checks first.  n == 0 passes (the callers then do nothing).
static int radiance_args(const pt_context* c, const pt_radiance_params* in, const void* rays, size_t n, const void* out,
                         pt_radiance_params* p) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  const int rp = radiance_params(in, p);
  if (rp) return rp;
  if (n > (size_t)ptd::kRaysMax) return fail(PT_ERR_INVALID, "more than 2^31 - 256 queries in one call");
  if (n > 0 && (!rays || !out)) return fail(PT_ERR_INVALID, "null argument");
  return PT_OK;
}

// plan_launch's choices for a launch of `paths` paths that is neither counted nor in stats mode and folds no
// moments: queries are none of these, whatever the context is set to for its renders.
static LaunchPlan radiance_plan(pt_context* c, long long paths) {
  const bool stats = c->stats_mode;
  const int count = c->opt_count, moments = c->opt_moments;
  c->stats_mode = false;
  c->opt_count = c->opt_moments = 0;
  const long long tiles = std::min<long long>((paths + 255) / 256, 1ll << 40);
  const LaunchPlan plan = plan_launch(*c, tiles, 1, false);
  c->stats_mode = stats;
  c->opt_count = count;
  c->opt_moments = moments;
  return plan;
}

extern "C" {

int pt_radiance_default_params(pt_radiance_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->n_samples = 1;
  out->seed_stride = 1;
  return PT_OK;
}

int pt_trace_radiance(pt_context* c, const pt_radiance_params* params, const void* d_rays, size_t n, void* d_out) {
  PT_SINGLE(c, "pt_trace_radiance");
  pt_radiance_params rp;
  const int ra = radiance_args(c, params, d_rays, n, d_out, &rp);
  if (ra) return ra;
  if (n == 0) return PT_OK;
  if (((uintptr_t)d_rays | (uintptr_t)d_out) & 15u) return fail(PT_ERR_INVALID, "device pointers must be 16-B aligned");
  {
    const uintptr_t r0 = (uintptr_t)d_rays, r1 = r0 + n * sizeof(pt_ray), o0 = (uintptr_t)d_out, o1 = o0 + n * 16;
    if (o0 < r1 && r0 < o1) return fail(PT_ERR_INVALID, "pt_trace_radiance: d_out overlaps d_rays");
  }
  PT_HIP(hipSetDevice(c->device));
  const long long S = rp.n_samples;
  const LaunchPlan plan = radiance_plan(c, (long long)n * S);
  if (plan.refuse) return fail(plan.refuse_code, plan.refuse);
  // the scene's, the lights' and the parameters' share of a render's parameters: a query has no frame and no camera
  ptd::RenderParams p{};
  p.nodes = c->d_nodes;
  p.n_nodes = c->n_nodes;
  p.tris = c->d_tris;
  p.hit_tris = c->d_tris;
  p.n_tris = c->n_tris;
  p.lights = c->d_lights_dev;
  p.n_lights = c->n_lights;
  p.stats = c->d_stats;   // never written: no kernel here counts
  p.max_depth = c->params.max_depth;
  p.sss_bounces = c->params.sss_bounces;
  p.exit_skip = plan.exit_skip;
  memcpy(p.root_lo, c->root_lo, sizeof p.root_lo);
  memcpy(p.root_hi, c->root_hi, sizeof p.root_hi);
  p.n_cull = -1;
  p.spl = 1;
  p.nranks = 1;
  p.wf_grid = c->opt_wf_grid;
  p.wide_refill = plan.wide_refill;
  if (plan.sweep) {   // render_params' rule
    p.sweep = c->opt_sweep_hull ? c->d_sweep : c->d_sweep_plain;
    p.sweep_hull = plan.sweep_hull;
    p.sweep_boxes = c->sweep_boxes;
    p.sweep_leaves = c->sweep_leaves;
    if (plan.sweep_cube) {
      p.sweep_cube = 1;
      memcpy(p.cube_under, c->cube_under, sizeof p.cube_under);
      p.cube_all = c->cube_all;
    }
  }
  // chunks of whole queries, at least one query each
  const long long want = c->opt_radiance_chunk > 0 ? c->opt_radiance_chunk : kRadianceAutoChunk;
  const long long per = std::min<long long>(std::max<long long>(1, want / S), (long long)n);   // queries a chunk
  const int ro = order_shared(c);   // the path buffers and the overflow areas are the context's
  if (ro) return ro;
  ptd::WfBuffers b{};
  if (plan.wf) {
    const int rb = radiance_wf_buffers(c, per * S, &b);
    if (rb) return rb;
    if (plan.wide) {
      const int rw = wide_params(c, &p);
      if (rw) return rw;
      p.wide_handback = plan.wide_handback;
      p.wf_fuse = plan.wf_fuse;
      p.wf_tail = plan.wf_tail;
    }
  } else {
    const int rg = grow_dev(c, &c->d_rad_colors, &c->rad_colors_cap, (size_t)(per * S));
    if (rg) return rg;
  }
  for (long long q0 = 0; q0 < (long long)n; q0 += per) {
    const long long nq = std::min(per, (long long)n - q0);
    if (plan.wf)
      PT_HIP(ptd::launch_wavefront_rays(p, b, plan.lds, d_rays, q0, nq, rp.n_samples, rp.seed_stride, d_out, c->stream));
    else
      PT_HIP(ptd::launch_radiance(p, plan.lds, d_rays, q0, nq, rp.n_samples, rp.seed_stride, c->d_rad_colors, d_out,
                                  c->stream));
  }
  accum_overwritten(c, d_out);
  return mark_shared(c);
}

int pt_trace_radiance_sync(pt_context* c, const pt_radiance_params* params, const pt_ray* rays, size_t n, float* out) {
  PT_SINGLE(c, "pt_trace_radiance_sync");
  pt_radiance_params rp;
  const int ra = radiance_args(c, params, rays, n, out, &rp);
  if (ra) return ra;
  if (n == 0) return PT_OK;
  PT_HIP(hipSetDevice(c->device));
  // in chunks, so that the staging buffers stay small beside a large batch
  const size_t chunk = std::min<size_t>(n, (size_t)1 << 21);
  typedef struct { char b[32]; } Rec;
  Rec* in = (Rec*)c->d_rad_in;
  int rg = grow_dev(c, &in, &c->rad_in_cap, chunk);
  c->d_rad_in = in;
  if (rg) return rg;
  rg = grow_dev(c, &c->d_rad_out, &c->rad_out_cap, chunk);
  if (rg) return rg;
  for (size_t i0 = 0; i0 < n; i0 += chunk) {
    const size_t m = std::min(chunk, n - i0);
    PT_HIP(hipMemcpyAsync(c->d_rad_in, rays + i0, m * sizeof(pt_ray), hipMemcpyHostToDevice, c->stream));
    const int rt = pt_trace_radiance(c, &rp, c->d_rad_in, m, c->d_rad_out);
    if (rt) return rt;
    PT_HIP(hipMemcpyAsync(out + 4 * i0, c->d_rad_out, m * 16, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
  }
  return PT_OK;
}

int pt_trace_radiance_host(const float* vertices, size_t n_vertex_floats, const uint32_t* indices, size_t n_indices,
                           const pt_bvh_node* nodes, size_t n_nodes, uint32_t flags, const pt_area_light* lights,
                           size_t n_lights, int max_depth, int sss_bounces, const pt_radiance_params* params,
                           const pt_ray* rays, size_t n, float* out, int threads) {
  if (!vertices || !indices || !nodes) return fail(PT_ERR_INVALID, "null scene array");
  if (n_lights > 0 && !lights) return fail(PT_ERR_INVALID, "null lights");
  if (max_depth < 0 || sss_bounces < 0) return fail(PT_ERR_INVALID, "max_depth and sss_bounces must be >= 0");
  pt_radiance_params rp;
  const int rc = radiance_params(params, &rp);
  if (rc) return rc;
  if (n > 0 && (!rays || !out)) return fail(PT_ERR_INVALID, "null argument");
  const std::string why = ptr::trace_radiance_host(
      vertices, n_vertex_floats, indices, n_indices, (const float*)nodes, n_nodes, (flags & PT_NODES_INT_BITS) != 0,
      (const float*)lights, n_lights, max_depth, sss_bounces, rp.n_samples, rp.seed_stride, (const float*)rays, n, out,
      threads);
  if (!why.empty()) return fail(PT_ERR_SCENE, why);
  return PT_OK;
}

int pt_camera_rays(pt_context* c, uint32_t batch, const int32_t* d_pixels, size_t n, void* d_rays) {
  PT_SINGLE(c, "pt_camera_rays");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->has_camera) return fail(PT_ERR_INVALID, "no camera set");
  if (c->width <= 0 || c->height <= 0) return fail(PT_ERR_INVALID, "no frame size (pt_resize_and_clear, pt_bind_accum)");
  if (n > (size_t)ptd::kRaysMax) return fail(PT_ERR_INVALID, "more than 2^31 - 256 rays in one call");
  if (!d_pixels && n > (size_t)c->width * (size_t)c->height)
    return fail(PT_ERR_INVALID, "pt_camera_rays: without a pixel list, n is at most width * height");
  if (n == 0) return PT_OK;
  if (!d_rays) return fail(PT_ERR_INVALID, "null argument");
  if (((uintptr_t)d_rays & 15u) || ((uintptr_t)d_pixels & 3u))
    return fail(PT_ERR_INVALID, "d_rays must be 16-B aligned, d_pixels 4-B");
  PT_HIP(hipSetDevice(c->device));
  ptd::RenderParams p{};
  p.width = c->width;
  p.height = c->height;
  camera_params(c->cam, &p);
  PT_HIP(ptd::launch_camera_rays(p, batch, d_pixels, (long long)n, d_rays, c->stream));
  accum_overwritten(c, d_rays);
  return note_use(c);
}

int pt_camera_rays_host(const float camera_ubo[16], int width, int height, uint32_t batch, const int32_t* pixels,
                        size_t n, pt_ray* rays) {
  if (!camera_ubo) return fail(PT_ERR_INVALID, "null camera");
  if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 31) - 256) return fail(PT_ERR_INVALID, "bad resolution");
  const size_t npx = (size_t)width * (size_t)height;
  if (!pixels && n > npx) return fail(PT_ERR_INVALID, "pt_camera_rays_host: without a pixel list, n is at most width * height");
  if (n > 0 && !rays) return fail(PT_ERR_INVALID, "null argument");
  for (size_t i = 0; pixels && i < n; ++i)
    if (pixels[i] < 0 || (size_t)pixels[i] >= npx)
      return fail(PT_ERR_INVALID, "pt_camera_rays_host: pixel " + std::to_string(i) + " lies outside the frame");
  ptr::camera_rays_host(camera_ubo, width, height, batch, pixels, n, (float*)rays);
  return PT_OK;
}

}  // extern "C"
