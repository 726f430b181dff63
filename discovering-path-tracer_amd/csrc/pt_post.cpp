// pt_post.cpp — the post-processing chain behind the C ABI (include/pathtracer.h):
// guide image, a-trous and variance-guided filters, moments readback, temporal
// reprojection and accumulation, spatial variance; the host statements
// (pt_*_host, pt_denoise.h) beside the device ones.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_denoise.h"
#include "pt_plan.h"

// Frees what this file allocates in a context (pt_destroy).
void post_release(pt_context* c) {
  dev_free(c->d_guide);
  dev_free(c->d_guide_prev);
  dev_free(c->d_dn_scratch[0]);
  dev_free(c->d_dn_scratch[1]);
  dev_free(c->d_denoised);
  dev_free(c->d_var[0]);
  dev_free(c->d_var[1]);
  dev_free(c->d_spatial_var);
  for (auto& s : c->tset) {
    dev_free(s.color);
    dev_free(s.moments);
    dev_free(s.length);
    dev_free(s.variance);
  }
}

// The caller's params, or the defaults for null.
template <class P>
static P params_or(const P* in, int (*defaults)(P*)) {
  if (in) return *in;
  P p;
  (void)defaults(&p);
  return p;
}

// The parameters of a guide launch for a width x height frame (pt_render_guide at the context's size,
// pt_upsample at the full one): the scene and the camera, the frame fields for that size, and the walk.
int guide_launch_params(pt_context* c, int width, int height, ptd::RenderParams* p, bool* lds) {
  frame_params(c, false, p);
  p->width = width;
  p->height = height;
  p->blocks_x = (width + 15) / 16;
  p->blocks_total = p->blocks_x * ((height + 15) / 16);
  p->n_cull = -1;
  // the wide walk first, then the LDS rule (pt_plan.h)
  const bool wide = c->opt_wide && c->n_wide > 0;
  const bool fits = lds_fits(*c, c->n_nodes);
  if (!wide && lds_refused(*c, fits)) return fail(PT_ERR_UNSUPPORTED, kLdsTooLarge);
  *lds = !wide && lds_staged(*c, fits);
  return wide ? wide_params(c, p) : PT_OK;
}

extern "C" {

// ---- first-hit guide image and a-trous denoiser (pt_denoise.h) --------------
int pt_denoise_default_params(pt_denoise_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->iterations = 5;
  out->sigma_color = 16.0f;
  out->sigma_normal = 0.35f;
  out->sigma_depth = 0.25f;
  return PT_OK;
}

static int denoise_params(const pt_denoise_params* in, pt_denoise_params* p) {
  *p = params_or(in, pt_denoise_default_params);
  if (!ptdn::params_ok(p->iterations, p->sigma_color, p->sigma_normal, p->sigma_depth))
    return fail(PT_ERR_INVALID, "pt_denoise_params: iterations 1-6; sigmas finite, > 0 and with a finite non-zero square");
  return PT_OK;
}

int pt_guide_ray(const float ubo[16], int w, int h, int x, int y, float o3[3], float d3[3]) {
  if (!ubo || !o3 || !d3) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0 || x < 0 || y < 0 || x >= w || y >= h) return fail(PT_ERR_INVALID, "pixel outside the frame");
  const ptdn::CamBasis b = ptdn::cam_basis(ubo);
  const ptm::v3 d = ptdn::guide_dir(b.dir, b.right, b.up, b.tan_fov, w, h, x, y);
  o3[0] = b.pos.x; o3[1] = b.pos.y; o3[2] = b.pos.z;
  d3[0] = d.x; d3[1] = d.y; d3[2] = d.z;
  return PT_OK;
}

int pt_denoise_host(const float* rgba, const float* guide, int w, int h, const pt_denoise_params* params, float* out) {
  if (!rgba || !guide || !out) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad resolution");
  pt_denoise_params p;
  const int rp = denoise_params(params, &p);
  if (rp) return rp;
  const size_t n = (size_t)w * (size_t)h;
  std::vector<float4> g(n), a(n), b(n);
  memcpy(g.data(), guide, n * sizeof(float4));
  memcpy(a.data(), rgba, n * sizeof(float4));
  for (int i = 0; i < p.iterations; ++i) {
    const ptdn::Sigma2 s = ptdn::pass_sigma2(p.sigma_color, p.sigma_normal, p.sigma_depth, i);
    const ptdn::ImageFetch fetch = {a.data(), g.data(), w};
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) b[(size_t)y * w + x] = ptdn::atrous_pixel(fetch, w, h, x, y, 1 << i, s);
    a.swap(b);
  }
  memcpy(out, a.data(), n * sizeof(float4));
  return PT_OK;
}

int pt_render_guide(pt_context* c) {
  PT_SINGLE(c, "pt_render_guide");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (!c->has_camera) return fail(PT_ERR_INVALID, "no camera set");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  PT_HIP(hipSetDevice(c->device));
  c->guide_valid = false;
  ptd::RenderParams p{};
  bool lds = false;
  const int rp = guide_launch_params(c, c->width, c->height, &p, &lds);
  if (rp) return rp;
  // the temporal history's guide is put aside before the image is written again (stream order keeps
  // whatever still reads it correct: only the pointers move)
  if (c->t_frames > 0 && !c->t_guide_aside && c->guide_serial == c->t_guide_serial) {
    std::swap(c->d_guide, c->d_guide_prev);
    std::swap(c->guide_cap, c->guide_prev_cap);
    c->t_guide_aside = true;
  }
  const int rg = grow_dev(c, &c->d_guide, &c->guide_cap, (size_t)c->width * c->height);
  if (rg) return rg;
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_guide(p, c->d_guide, lds, c->stream));
  c->guide_serial++;
  c->guide_valid = true;
  return mark_shared(c);
}

void* pt_guide_device_ptr(pt_context* c) {
  if (!c || c->group || !c->guide_valid) return nullptr;
  return (void*)c->d_guide;
}

int pt_read_guide(pt_context* c, float* out, size_t n) {
  PT_SINGLE(c, "pt_read_guide");
  if (!c || !out) return fail(PT_ERR_INVALID, "null argument");
  if (!c->guide_valid) return fail(PT_ERR_INVALID, "no guide image for the current scene, camera and size (pt_render_guide)");
  return read_image(c, c->d_guide, c->width, c->height, 4, out, n);
}

int pt_denoise(pt_context* c, const pt_denoise_params* params, const void* src, void* dst) {
  PT_SINGLE(c, "pt_denoise");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_denoise_params p;
  const int rp = denoise_params(params, &p);
  if (rp) return rp;
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (!c->has_camera) return fail(PT_ERR_INVALID, "no camera set");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  if ((((uintptr_t)src) & 15) || (((uintptr_t)dst) & 15)) return fail(PT_ERR_INVALID, "images must be 16-B aligned");
  const float4* in = src ? (const float4*)src : c->d_accum;
  if (dst && (const float4*)dst == in) return fail(PT_ERR_INVALID, "pt_denoise: source and destination must differ");
  PT_HIP(hipSetDevice(c->device));
  if (!c->guide_valid) {
    const int rg = pt_render_guide(c);
    if (rg) return rg;
  }
  const int w = c->width, h = c->height;
  const size_t n = (size_t)w * h;
  for (int k = 0; k < 2 && k < p.iterations - 1; ++k) {   // the ping-pong images the passes need
    const int rs = grow_dev(c, &c->d_dn_scratch[k], &c->dn_scratch_cap[k], n);
    if (rs) return rs;
  }
  float4* out = (float4*)dst;
  if (!out) {
    c->denoised_w = c->denoised_h = 0;
    const int rd = grow_dev(c, &c->d_denoised, &c->denoised_cap, n);
    if (rd) return rd;
    out = c->d_denoised;
  }
  const int ro = order_shared(c);
  if (ro) return ro;
  // pass i reads the previous pass's image (the source first) and writes a
  // scratch image, the last one the destination; the source is only read
  const float4* cur = in;
  for (int i = 0; i < p.iterations; ++i) {
    float4* to = i == p.iterations - 1 ? out : c->d_dn_scratch[i & 1];
    const ptdn::Sigma2 s = ptdn::pass_sigma2(p.sigma_color, p.sigma_normal, p.sigma_depth, i);
    PT_HIP(ptd::launch_atrous(cur, c->d_guide, to, w, h, 1 << i, s.c, s.n, s.z, c->opt_denoise_lds != 0 && i < 2,
                              c->stream));
    cur = to;
  }
  if (!dst) {
    c->denoised_w = w;
    c->denoised_h = h;
  }
  accum_overwritten(c, out);
  return mark_shared(c);
}

int pt_read_denoised(pt_context* c, float* rgba, size_t n) {
  PT_SINGLE(c, "pt_read_denoised");
  if (!c || !rgba) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_denoised || c->denoised_w == 0)
    return fail(PT_ERR_INVALID, "no library-owned denoised image (pt_denoise with a null destination)");
  return read_image(c, c->d_denoised, c->denoised_w, c->denoised_h, 4, rgba, n);
}

// ---- luminance moments and the variance-guided filter (pt_denoise.h) --------
static bool moments_ready(const pt_context* c) {
  return c->opt_moments && c->moments_valid && c->d_moments && c->moments_n >= 1;
}

void* pt_moments_device_ptr(pt_context* c) {
  if (!c || c->group || !moments_ready(c)) return nullptr;
  return (void*)c->d_moments;
}

int pt_read_moments(pt_context* c, float* out, size_t n, uint32_t* n_samples) {
  PT_SINGLE(c, "pt_read_moments");
  if (!c || !out) return fail(PT_ERR_INVALID, "null argument");
  if (!c->opt_moments || !c->d_moments || c->moments_cap < (size_t)c->width * c->height)
    return fail(PT_ERR_INVALID, "no moments image (PT_OPT_MOMENTS, then a render)");
  const int rr = read_image(c, c->d_moments, c->width, c->height, 2, out, n);
  if (rr) return rr;
  if (n_samples) *n_samples = moments_ready(c) ? c->moments_n : 0u;   // 0: not batches 0..n-1 in order
  return PT_OK;
}

int pt_denoise_var_default_params(pt_denoise_var_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->iterations = 4;
  out->sigma_lum = 1.5f;
  out->sigma_normal = 1.0f;
  out->sigma_depth = 1.0f;
  return PT_OK;
}

static int denoise_var_params(const pt_denoise_var_params* in, pt_denoise_var_params* p) {
  *p = params_or(in, pt_denoise_var_default_params);
  if (!ptdn::var_params_ok(p->iterations, p->sigma_lum, p->sigma_normal, p->sigma_depth))
    return fail(PT_ERR_INVALID, "pt_denoise_var_params: iterations 1-6; sigmas finite, > 0 and with a finite non-zero square");
  return PT_OK;
}

int pt_denoise_var_host(const float* rgba, const float* moments, uint32_t n_samples, const float* guide, int w, int h,
                        const pt_denoise_var_params* params, float* out) {
  if (!rgba || !moments || !guide || !out) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad resolution");
  if (n_samples < 2) return fail(PT_ERR_INVALID, "pt_denoise_var: the variance of the mean needs at least 2 samples");
  const size_t n = (size_t)w * (size_t)h;
  std::vector<float> va(n);
  for (size_t i = 0; i < n; ++i) va[i] = ptdn::var_of_mean(moments[2 * i], moments[2 * i + 1], n_samples);
  return pt_denoise_var_plane_host(rgba, va.data(), guide, w, h, params, out);
}

int pt_denoise_var_plane_host(const float* rgba, const float* variance, const float* guide, int w, int h,
                              const pt_denoise_var_params* params, float* out) {
  if (!rgba || !variance || !guide || !out) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad resolution");
  pt_denoise_var_params p;
  const int rp = denoise_var_params(params, &p);
  if (rp) return rp;
  const size_t n = (size_t)w * (size_t)h;
  std::vector<float4> g(n), a(n), b(n);
  std::vector<float> va(variance, variance + n), vb(n);
  memcpy(g.data(), guide, n * sizeof(float4));
  memcpy(a.data(), rgba, n * sizeof(float4));
  const float sn2 = p.sigma_normal * p.sigma_normal, sz2 = p.sigma_depth * p.sigma_depth;
  for (int i = 0; i < p.iterations; ++i) {
    const ptdn::VarImageFetch fetch = {a.data(), g.data(), va.data(), w};
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const ptdn::VarOut o = ptdn::atrous_var_pixel(fetch, w, h, x, y, 1 << i, p.sigma_lum, sn2, sz2);
        b[(size_t)y * w + x] = o.c;
        vb[(size_t)y * w + x] = o.v;
      }
    a.swap(b);
    va.swap(vb);
  }
  memcpy(out, a.data(), n * sizeof(float4));
  return PT_OK;
}

static int var_filter(pt_context* c, const pt_denoise_var_params& p, const float4* src, const float* var0,
                      const float4* guide, float4* dst);

int pt_denoise_var(pt_context* c, const pt_denoise_var_params* params, void* dst) {
  PT_SINGLE(c, "pt_denoise_var");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_denoise_var_params p;
  const int rp = denoise_var_params(params, &p);
  if (rp) return rp;
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (!c->has_camera) return fail(PT_ERR_INVALID, "no camera set");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  if (!moments_ready(c)) return fail(PT_ERR_INVALID, "pt_denoise_var: no valid moments (PT_OPT_MOMENTS, then a render from batch 0)");
  if (c->moments_n < 2) return fail(PT_ERR_INVALID, "pt_denoise_var: the variance of the mean needs at least 2 samples");
  if (((uintptr_t)dst) & 15) return fail(PT_ERR_INVALID, "images must be 16-B aligned");
  if (dst && (float4*)dst == c->d_accum) return fail(PT_ERR_INVALID, "pt_denoise_var: source and destination must differ");
  PT_HIP(hipSetDevice(c->device));
  if (!c->guide_valid) {
    const int rg = pt_render_guide(c);
    if (rg) return rg;
  }
  return var_filter(c, p, c->d_accum, nullptr, c->d_guide, (float4*)dst);
}

// The variance-guided filter's passes of the context's frame: from colour src, the guide and either the
// variance plane var0 (only read) or, var0 null, the variance of the mean of the context's moments.
// dst null: the library-owned image pt_read_denoised reads.
static int var_filter(pt_context* c, const pt_denoise_var_params& p, const float4* src, const float* var0,
                      const float4* guide, float4* dst) {
  const int w = c->width, h = c->height;
  const size_t n = (size_t)w * h;
  for (int k = 0; k < 2 && k < p.iterations - 1; ++k) {
    const int rs = grow_dev(c, &c->d_dn_scratch[k], &c->dn_scratch_cap[k], n);
    if (rs) return rs;
  }
  for (int k = 0; k < 2; ++k) {   // the variance planes: var0 in [0], pass i from [i & 1] to [(i + 1) & 1]
    const int rv = grow_dev(c, &c->d_var[k], &c->var_cap[k], n);
    if (rv) return rv;
  }
  float4* out = (float4*)dst;
  if (!out) {
    c->denoised_w = c->denoised_h = 0;
    const int rd = grow_dev(c, &c->d_denoised, &c->denoised_cap, n);
    if (rd) return rd;
    out = c->d_denoised;
  }
  const int ro = order_shared(c);
  if (ro) return ro;
  if (!var0) PT_HIP(ptd::launch_moments_var(c->d_moments, c->d_var[0], w, h, c->moments_n, c->stream));
  const float sn2 = p.sigma_normal * p.sigma_normal, sz2 = p.sigma_depth * p.sigma_depth;
  const float4* cur = src;
  for (int i = 0; i < p.iterations; ++i) {
    float4* to = i == p.iterations - 1 ? out : c->d_dn_scratch[i & 1];
    const float* vsrc = i == 0 && var0 ? var0 : c->d_var[i & 1];
    PT_HIP(ptd::launch_atrous_var(cur, vsrc, guide, to, c->d_var[(i + 1) & 1], w, h, 1 << i, p.sigma_lum, sn2, sz2,
                                  c->opt_denoise_lds != 0 && i < 2, c->stream));
    cur = to;
  }
  if (!dst) {
    c->denoised_w = w;
    c->denoised_h = h;
  }
  return mark_shared(c);
}

// ---- temporal reprojection (pt_denoise.h reproject_pixel) --------------------
int pt_temporal_default_params(pt_temporal_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->max_history = 64;
  out->alpha_min = 0.0f;
  out->normal_min = 0.5f;
  out->depth_rel = 0.05f;
  return PT_OK;
}

static int temporal_params(const pt_temporal_params* in, pt_temporal_params* p) {
  *p = params_or(in, pt_temporal_default_params);
  if (!ptdn::temporal_params_ok(p->max_history, p->alpha_min, p->normal_min, p->depth_rel))
    return fail(PT_ERR_INVALID,
                "pt_temporal_params: max_history 1-65536, alpha_min in [0, 1], normal_min in [-1, 1], depth_rel finite and > 0");
  return PT_OK;
}

// The checks pt_reproject and pt_reproject_host share: sizes, the sample count, the images' presence (the
// history all there or all null) and that no output is an input or another output.
static int reproject_args(const float* cam_cur, const float* cam_prev, int w, int h, uint32_t n,
                          const pt_reproject_images* im) {
  if (!cam_cur || !cam_prev || !im) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 31)) return fail(PT_ERR_INVALID, "bad resolution");
  if (n < 1 || n > 65536) return fail(PT_ERR_INVALID, "pt_reproject: n takes 1 to 65536 samples");
  if (!im->color || !im->moments || !im->guide || !im->out_color || !im->out_moments || !im->out_length ||
      !im->out_variance)
    return fail(PT_ERR_INVALID, "pt_reproject: null image");
  const int nh = (im->hist_color ? 1 : 0) + (im->hist_moments ? 1 : 0) + (im->hist_length ? 1 : 0) + (im->hist_guide ? 1 : 0);
  if (nh != 0 && nh != 4) return fail(PT_ERR_INVALID, "pt_reproject: the four history images are all given or all null");
  const void* in[7] = {im->color, im->moments, im->guide, im->hist_color, im->hist_moments, im->hist_length, im->hist_guide};
  const void* out[4] = {im->out_color, im->out_moments, im->out_length, im->out_variance};
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 7; ++k)
      if (out[i] == in[k]) return fail(PT_ERR_INVALID, "pt_reproject: an output image is also an input");
    for (int k = 0; k < i; ++k)
      if (out[i] == out[k]) return fail(PT_ERR_INVALID, "pt_reproject: two output images are the same");
  }
  return PT_OK;
}

int pt_reproject_host(const float cam_cur[16], const float cam_prev[16], int w, int h, uint32_t n,
                      const pt_reproject_images* im, const pt_temporal_params* params) {
  const int ra = reproject_args(cam_cur, cam_prev, w, h, n, im);
  if (ra) return ra;
  pt_temporal_params p;
  const int rp = temporal_params(params, &p);
  if (rp) return rp;
  const size_t np = (size_t)w * (size_t)h;
  std::vector<float4> hc, hg;
  std::vector<float2> hm;
  ptdn::HistImages hist = {nullptr, nullptr, nullptr, nullptr};
  if (im->hist_color) {
    hc.resize(np);
    hg.resize(np);
    hm.resize(np);
    memcpy(hc.data(), im->hist_color, np * sizeof(float4));
    memcpy(hg.data(), im->hist_guide, np * sizeof(float4));
    memcpy(hm.data(), im->hist_moments, np * sizeof(float2));
    hist = {hc.data(), hm.data(), im->hist_length, hg.data()};
  }
  const ptdn::CamBasis B = ptdn::cam_basis(cam_cur), Bp = ptdn::cam_basis(cam_prev);
  const ptdn::TemporalParams tp = {(float)p.max_history, p.alpha_min, p.normal_min, p.depth_rel};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      float4 c, g;
      float2 m;
      memcpy(&c, im->color + 4 * i, sizeof c);
      memcpy(&g, im->guide + 4 * i, sizeof g);
      memcpy(&m, im->moments + 2 * i, sizeof m);
      const ptdn::ReprojOut o = ptdn::reproject_pixel(hist, B, Bp, w, h, x, y, c, m, g, (float)n, tp);
      memcpy(im->out_color + 4 * i, &o.c, sizeof o.c);
      memcpy(im->out_moments + 2 * i, &o.m, sizeof o.m);
      im->out_length[i] = o.len;
      im->out_variance[i] = o.var;
    }
  return PT_OK;
}

// The reprojection of checked device images with validated params, on the context's stream.
static int reproject_launch(pt_context* c, const pt_reproject_images& im, const float cam_cur[16],
                            const float cam_prev[16], int w, int h, uint32_t n, const pt_temporal_params& p) {
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_reproject((const float4*)im.color, (const float2*)im.moments, (const float4*)im.guide,
                               (const float4*)im.hist_color, (const float2*)im.hist_moments, im.hist_length,
                               (const float4*)im.hist_guide, (float4*)im.out_color, (float2*)im.out_moments,
                               im.out_length, im.out_variance, cam_cur, cam_prev, w, h, n, p.max_history, p.alpha_min,
                               p.normal_min, p.depth_rel, c->stream));
  accum_overwritten(c, im.out_color);
  return mark_shared(c);
}

int pt_reproject(pt_context* c, const float cam_cur[16], const float cam_prev[16], int w, int h, uint32_t n,
                 const pt_reproject_images* im, const pt_temporal_params* params) {
  PT_SINGLE(c, "pt_reproject");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  const int ra = reproject_args(cam_cur, cam_prev, w, h, n, im);
  if (ra) return ra;
  pt_temporal_params p;
  const int rp = temporal_params(params, &p);
  if (rp) return rp;
  const uintptr_t a16 = (uintptr_t)im->color | (uintptr_t)im->guide | (uintptr_t)im->hist_color |
                        (uintptr_t)im->hist_guide | (uintptr_t)im->out_color;
  const uintptr_t a8 = (uintptr_t)im->moments | (uintptr_t)im->hist_moments | (uintptr_t)im->out_moments;
  const uintptr_t a4 = (uintptr_t)im->hist_length | (uintptr_t)im->out_length | (uintptr_t)im->out_variance;
  if ((a16 & 15) || (a8 & 7) || (a4 & 3))
    return fail(PT_ERR_INVALID, "pt_reproject: colours and guides must be 16-B aligned, moments 8-B, lengths and variance 4-B");
  PT_HIP(hipSetDevice(c->device));
  return reproject_launch(c, *im, cam_cur, cam_prev, w, h, n, p);
}

// One image set of at least n pixels.
static int grow_tset(pt_context* c, pt_context::TemporalSet* s, size_t n) {
  if (s->color && s->cap >= n) return PT_OK;
  s->cap = 0;
  size_t cap[4] = {0, 0, 0, 0};   // the four images grow together
  int rc = grow_dev(c, &s->color, &cap[0], n);
  if (!rc) rc = grow_dev(c, &s->moments, &cap[1], n);
  if (!rc) rc = grow_dev(c, &s->length, &cap[2], n);
  if (!rc) rc = grow_dev(c, &s->variance, &cap[3], n);
  if (!rc) s->cap = n;
  return rc;
}

static const char* temporal_unsupported(const pt_context* c) {
  if (c->nranks > 1) return "not on a partition of more than one rank";
  if (c->stats_mode) return "not in stats mode";
  if (c->opt_count) return "not with PT_OPT_COUNT_TRACED";
  return nullptr;
}

int pt_temporal_advance(pt_context* c, const float ubo[16], uint32_t n_batches) {
  PT_SINGLE(c, "pt_temporal_advance");
  if (!c || !ubo) return fail(PT_ERR_INVALID, "null argument");
  if (const char* why = temporal_unsupported(c)) return fail(PT_ERR_UNSUPPORTED, std::string("pt_temporal_advance: ") + why);
  if (n_batches < 1 || n_batches > 65536) return fail(PT_ERR_INVALID, "pt_temporal_advance: n_batches takes 1 to 65536");
  if (!c->opt_moments) return fail(PT_ERR_INVALID, "pt_temporal_advance: needs PT_OPT_MOMENTS 1");
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (c->n_lights < 1) return fail(PT_ERR_INVALID, "no lights uploaded");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  PT_HIP(hipSetDevice(c->device));
  const int w = c->width, h = c->height;
  const size_t n = (size_t)w * h;
  const bool have = c->t_frames > 0 && c->t_w == w && c->t_h == h;
  if (!have) temporal_forget(c);
  const int dst = have ? 1 - c->t_cur : 0;
  {
    const int rs = grow_tset(c, &c->tset[dst], n);
    if (rs) return rs;
  }
  int rc = pt_set_camera(c, ubo);
  if (rc) return rc;
  rc = pt_clear_accum(c);
  if (rc) return rc;
  c->seed_extra = c->t_samples;
  rc = render_impl(c, 0, n_batches, nullptr);
  c->seed_extra = 0;
  if (rc) return rc;
  rc = pt_render_guide(c);   // puts the last frame's guide aside first
  if (rc) return rc;
  const pt_context::TemporalSet& src = c->tset[c->t_cur];
  const pt_context::TemporalSet& out = c->tset[dst];
  const float4* hist_guide = c->t_guide_aside ? c->d_guide_prev : nullptr;
  const bool hist = have && hist_guide;
  pt_temporal_params p;
  (void)pt_temporal_default_params(&p);
  const pt_reproject_images im = {(const float*)c->d_accum, (const float*)c->d_moments, (const float*)c->d_guide,
                                  hist ? (const float*)src.color : nullptr, hist ? (const float*)src.moments : nullptr,
                                  hist ? src.length : nullptr, hist ? (const float*)hist_guide : nullptr,
                                  (float*)out.color, (float*)out.moments, out.length, out.variance};
  rc = reproject_launch(c, im, ubo, c->t_cam, w, h, n_batches, p);
  if (rc) return rc;
  c->t_cur = dst;
  c->t_frames++;
  c->t_samples += n_batches;
  memcpy(c->t_cam, ubo, sizeof c->t_cam);
  c->t_w = w;
  c->t_h = h;
  c->t_guide_serial = c->guide_serial;
  c->t_guide_aside = false;
  return PT_OK;
}

int pt_temporal_reset(pt_context* c) {
  PT_SINGLE(c, "pt_temporal_reset");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  temporal_forget(c);
  return PT_OK;
}

int pt_temporal_info(pt_context* c, uint32_t* frames, uint32_t* samples) {
  PT_SINGLE(c, "pt_temporal_info");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (frames) *frames = c->t_frames;
  if (samples) *samples = c->t_samples;
  return PT_OK;
}

// Whether the context holds a temporal result of the current frame size.
static bool temporal_ready(const pt_context* c) {
  return c->t_frames > 0 && c->t_w == c->width && c->t_h == c->height && c->tset[c->t_cur].color;
}

void* pt_temporal_device_ptr(pt_context* c, int which) {
  if (!c || c->group || !temporal_ready(c)) return nullptr;
  const pt_context::TemporalSet& s = c->tset[c->t_cur];
  return which == 0 ? (void*)s.color : which == 1 ? (void*)s.moments : which == 2 ? (void*)s.length
         : which == 3 ? (void*)s.variance : nullptr;
}

int pt_read_temporal(pt_context* c, float* rgba, float* moments, float* length) {
  PT_SINGLE(c, "pt_read_temporal");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!temporal_ready(c)) return fail(PT_ERR_INVALID, "no temporal result for the current frame (pt_temporal_advance)");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  const pt_context::TemporalSet& s = c->tset[c->t_cur];
  const size_t n = (size_t)c->t_w * c->t_h;
  if (rgba) PT_HIP(hipMemcpyAsync(rgba, s.color, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  if (moments) PT_HIP(hipMemcpyAsync(moments, s.moments, n * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
  if (length) PT_HIP(hipMemcpyAsync(length, s.length, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  PT_HIP(hipStreamSynchronize(c->stream));
  return PT_OK;
}

// ---- spatial variance of short histories (pt_denoise.h spatial_var_pixel) ----
int pt_spatial_var_default_params(pt_spatial_var_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->below = 2;
  out->radius = 1;
  out->sigma_normal = 1.0f;
  out->sigma_depth = 0.5f;
  return PT_OK;
}

static int spatial_var_params(const pt_spatial_var_params* in, pt_spatial_var_params* p) {
  *p = params_or(in, pt_spatial_var_default_params);
  if (!ptdn::spatial_params_ok(p->below, p->radius, p->sigma_normal, p->sigma_depth))
    return fail(PT_ERR_INVALID,
                "pt_spatial_var_params: below 0-65536, radius 1-3; sigmas finite, > 0 and with a finite non-zero square");
  return PT_OK;
}

// The checks pt_spatial_variance and pt_spatial_variance_host share.
static int spatial_var_args(const void* moments, const void* length, const void* variance, const void* guide, int w,
                            int h, const void* out) {
  if (!moments || !length || !variance || !guide || !out) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 31)) return fail(PT_ERR_INVALID, "bad resolution");
  if (out == moments || out == length || out == variance || out == guide)
    return fail(PT_ERR_INVALID, "pt_spatial_variance: the output is also an input");
  return PT_OK;
}

int pt_spatial_variance_host(const float* moments, const float* length, const float* variance, const float* guide,
                             int w, int h, const pt_spatial_var_params* params, float* out) {
  const int ra = spatial_var_args(moments, length, variance, guide, w, h, out);
  if (ra) return ra;
  pt_spatial_var_params p;
  const int rp = spatial_var_params(params, &p);
  if (rp) return rp;
  const size_t n = (size_t)w * (size_t)h;
  std::vector<float2> m(n);
  std::vector<float4> g(n);
  memcpy(m.data(), moments, n * sizeof(float2));
  memcpy(g.data(), guide, n * sizeof(float4));
  const ptdn::SpatialImageFetch fetch = {m.data(), length, g.data(), w};
  const float below = (float)p.below;
  const float sn2 = p.sigma_normal * p.sigma_normal, sz2 = p.sigma_depth * p.sigma_depth;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      const float lenp = length[i];
      out[i] = lenp < below ? ptdn::spatial_var_pixel(fetch, w, h, x, y, p.radius, sn2, sz2, g[i], lenp) : variance[i];
    }
  return PT_OK;
}

int pt_spatial_variance(pt_context* c, const void* moments, const void* length, const void* variance,
                        const void* guide, int w, int h, const pt_spatial_var_params* params, void* out) {
  PT_SINGLE(c, "pt_spatial_variance");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  const int ra = spatial_var_args(moments, length, variance, guide, w, h, out);
  if (ra) return ra;
  pt_spatial_var_params p;
  const int rp = spatial_var_params(params, &p);
  if (rp) return rp;
  if (((uintptr_t)moments & 7) || (((uintptr_t)length | (uintptr_t)variance | (uintptr_t)out) & 3) || ((uintptr_t)guide & 15))
    return fail(PT_ERR_INVALID, "pt_spatial_variance: moments must be 8-B aligned, the guide 16-B, length, variance and out 4-B");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_spatial_var((const float2*)moments, (const float*)length, (const float*)variance,
                                 (const float4*)guide, (float*)out, w, h, p.below, p.radius,
                                 p.sigma_normal * p.sigma_normal, p.sigma_depth * p.sigma_depth, c->stream));
  accum_overwritten(c, out);
  return mark_shared(c);
}

// ---- the variance-guided filter of the temporal result ------------------------------
// The guide of the current temporal frame: still d_guide, or where a later pt_render_guide put it
// aside; null when it is gone.
static const float4* temporal_guide(const pt_context* c) {
  return c->t_guide_aside ? c->d_guide_prev : c->guide_serial == c->t_guide_serial ? c->d_guide : nullptr;
}

// pt_temporal_denoise (sp null) and pt_temporal_denoise_spatial behind their argument checks: the
// filter of the temporal colour from its variance plane, or from the plane with the short histories'
// variance estimated spatially first (sp).  name: the entry point, for the messages.
static int temporal_filter(pt_context* c, const pt_denoise_var_params& p, const pt_spatial_var_params* sp, void* dst,
                           const char* name) {
  if (!temporal_ready(c)) return fail(PT_ERR_INVALID, "no temporal result for the current frame (pt_temporal_advance)");
  if (((uintptr_t)dst) & 15) return fail(PT_ERR_INVALID, "images must be 16-B aligned");
  const pt_context::TemporalSet& s = c->tset[c->t_cur];
  if (dst && (float4*)dst == s.color)
    return fail(PT_ERR_INVALID, std::string(name) + ": source and destination must differ");
  const float4* guide = temporal_guide(c);
  if (!guide) return fail(PT_ERR_INVALID, std::string(name) + ": the temporal frame's guide is gone");
  PT_HIP(hipSetDevice(c->device));
  const float* variance = s.variance;
  if (sp) {
    const int w = c->width, h = c->height;
    const int rg = grow_dev(c, &c->d_spatial_var, &c->spatial_var_cap, (size_t)w * h);
    if (rg) return rg;
    const int ro = order_shared(c);
    if (ro) return ro;
    PT_HIP(ptd::launch_spatial_var(s.moments, s.length, s.variance, guide, c->d_spatial_var, w, h, sp->below,
                                   sp->radius, sp->sigma_normal * sp->sigma_normal,
                                   sp->sigma_depth * sp->sigma_depth, c->stream));
    const int rm = mark_shared(c);
    if (rm) return rm;
    variance = c->d_spatial_var;
  }
  const int rf = var_filter(c, p, s.color, variance, guide, (float4*)dst);
  if (rf) return rf;
  accum_overwritten(c, dst);
  return PT_OK;
}

int pt_temporal_denoise(pt_context* c, const pt_denoise_var_params* params, void* dst) {
  PT_SINGLE(c, "pt_temporal_denoise");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_denoise_var_params p;
  const int rp = denoise_var_params(params, &p);
  if (rp) return rp;
  return temporal_filter(c, p, nullptr, dst, "pt_temporal_denoise");
}

int pt_temporal_denoise_spatial(pt_context* c, const pt_denoise_var_params* params,
                                const pt_spatial_var_params* spatial, void* dst) {
  PT_SINGLE(c, "pt_temporal_denoise_spatial");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_denoise_var_params p;
  const int rp = denoise_var_params(params, &p);
  if (rp) return rp;
  pt_spatial_var_params sp;
  const int rs = spatial_var_params(spatial, &sp);
  if (rs) return rs;
  return temporal_filter(c, p, &sp, dst, "pt_temporal_denoise_spatial");
}

}  // extern "C"

// ---- for pt_adaptive.cpp (pt_adaptive_denoise) ------------------------------------------
int post_var_filter(pt_context* c, const pt_denoise_var_params& p, const float4* src, const float* var0,
                    const float4* guide, float4* dst) {
  return var_filter(c, p, src, var0, guide, dst);
}
int post_denoise_var_params(const pt_denoise_var_params* in, pt_denoise_var_params* p) {
  return denoise_var_params(in, p);
}
