// pt_upsample.cpp — guide-driven upsampling behind the C ABI (include/pathtracer.h):
// a frame rendered at 1/s of the size onto the full grid under the full-size
// guide's edge stop, as float4 or fused with the display transform; the
// full-size guide the context keeps for it; the host statement
// (pt_upsample_host, pt_upsample.h) beside them.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_upsample.h"

// Frees what this file allocates in a context (pt_destroy).
void upsample_release(pt_context* c) {
  dev_free(c->d_up_guide);
  dev_free(c->d_upsampled);
  dev_free(c->d_up_display);
}

static int upsample_params(const pt_upsample_params* in, pt_upsample_params* p) {
  if (in) *p = *in;
  else (void)pt_upsample_default_params(p);
  if (!ptup::params_ok(p->scale, p->sigma_normal, p->sigma_depth))
    return fail(PT_ERR_INVALID, "pt_upsample_params: scale 2-8; sigmas finite, > 0 and with a finite non-zero square");
  return PT_OK;
}

// The low size and the scale: the full frame has at most 2^31 pixels and 65535 rows of tiles.
static int upsample_size(int w, int h, int s) {
  if (!ptup::size_ok(w, h, s) || ((long long)h * s + 15) / 16 > 65535)
    return fail(PT_ERR_INVALID, "bad resolution: the full frame (scale * w) x (scale * h) holds at most 2^31 pixels");
  return PT_OK;
}

static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  return (const char*)a < (const char*)b + b_bytes && (const char*)b < (const char*)a + a_bytes;
}

// The checks of the device images: src w x h float4, guide (null: the library's own) and dst full size, dst
// (if the caller's) of dst_px bytes a pixel.
static int upsample_images_ok(const void* src, const void* guide, const void* dst, int w, int h, int s,
                              size_t dst_px) {
  if ((((uintptr_t)src | (uintptr_t)guide) & 15) || (((uintptr_t)dst) & (dst_px - 1)))
    return fail(PT_ERR_INVALID, dst_px == 16 ? "images must be 16-B aligned"
                                             : "the source and the guide must be 16-B aligned, the destination 4-B");
  if (!dst) return PT_OK;
  const size_t n = (size_t)w * h, N = n * s * s;
  if (overlap(dst, N * dst_px, src, n * sizeof(float4)) || (guide && overlap(dst, N * dst_px, guide, N * sizeof(float4))))
    return fail(PT_ERR_INVALID, "the destination must not overlap the source or the guide");
  return PT_OK;
}

static bool up_guide_current(const pt_context* c, int s) {
  return c->d_up_guide && s != 0 && c->up_scale == s && c->up_w == c->width && c->up_h == c->height && c->has_camera &&
         memcmp(c->up_cam, c->cam, sizeof c->cam) == 0;
}

// The full-size guide of the context's scene and camera at scale s: kept, or rendered as
// pt_render_guide renders the context's own (which is not touched).
static int upsample_guide(pt_context* c, int s) {
  if (up_guide_current(c, s)) return PT_OK;
  c->up_scale = 0;
  const int W = c->width * s, H = c->height * s;
  ptd::RenderParams p{};
  bool lds = false;
  const int rp = guide_launch_params(c, W, H, &p, &lds);
  if (rp) return rp;
  const int rg = grow_dev(c, &c->d_up_guide, &c->up_guide_cap, (size_t)W * H);
  if (rg) return rg;
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_guide(p, c->d_up_guide, lds, c->stream));
  c->up_guide_launches++;
  c->up_scale = s;
  c->up_w = c->width;
  c->up_h = c->height;
  memcpy(c->up_cam, c->cam, sizeof c->up_cam);
  return mark_shared(c);
}

// What pt_upsample and pt_upsample_display ask of the context beside the images.
static int upsample_context_ok(pt_context* c) {
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (!c->has_camera) return fail(PT_ERR_INVALID, "no camera set");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  return PT_OK;
}

// The float kernel's launch of checked images; dst null: the library-owned image.
static int upsample_launch(pt_context* c, const pt_upsample_params& p, const float4* src, int w, int h,
                           const float4* guide, float4* dst) {
  const int W = w * p.scale, H = h * p.scale;
  float4* out = dst;
  if (!out) {
    c->upsampled_w = c->upsampled_h = 0;
    const int rd = grow_dev(c, &c->d_upsampled, &c->upsampled_cap, (size_t)W * H);
    if (rd) return rd;
    out = c->d_upsampled;
  }
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_upsample(src, guide, out, w, h, p.scale, p.sigma_normal * p.sigma_normal,
                              p.sigma_depth * p.sigma_depth, c->stream));
  if (!dst) {
    c->upsampled_w = W;
    c->upsampled_h = H;
  }
  accum_overwritten(c, out);
  return mark_shared(c);
}

extern "C" {

int pt_upsample_default_params(pt_upsample_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->scale = 2;
  out->sigma_normal = 0.35f;
  out->sigma_depth = 0.25f;
  return PT_OK;
}

int pt_upsample_host(const float* src, int w, int h, const float* guide_full, const pt_upsample_params* params,
                     float* out) {
  if (!src || !guide_full || !out) return fail(PT_ERR_INVALID, "null argument");
  pt_upsample_params p;
  const int rp = upsample_params(params, &p);
  if (rp) return rp;
  const int rs = upsample_size(w, h, p.scale);
  if (rs) return rs;
  const int W = w * p.scale, H = h * p.scale;
  const size_t n = (size_t)w * h, N = (size_t)W * H;
  std::vector<float4> c(n), g(N);
  memcpy(c.data(), src, n * sizeof(float4));
  memcpy(g.data(), guide_full, N * sizeof(float4));
  const ptup::Frame f = {w, h, p.scale, p.sigma_normal * p.sigma_normal, p.sigma_depth * p.sigma_depth};
  for (int Y = 0; Y < H; ++Y)
    for (int X = 0; X < W; ++X) {
      const float4 o = ptup::upsample_pixel(c.data(), g.data(), f, X, Y);
      memcpy(out + 4 * ((size_t)Y * W + X), &o, sizeof o);
    }
  return PT_OK;
}

int pt_upsample_images(pt_context* c, const pt_upsample_params* params, const void* src, int w, int h,
                       const void* guide_full, void* dst) {
  PT_SINGLE(c, "pt_upsample_images");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!src || !guide_full) return fail(PT_ERR_INVALID, "null argument");
  pt_upsample_params p;
  const int rp = upsample_params(params, &p);
  if (rp) return rp;
  const int rs = upsample_size(w, h, p.scale);
  if (rs) return rs;
  const int ri = upsample_images_ok(src, guide_full, dst, w, h, p.scale, sizeof(float4));
  if (ri) return ri;
  PT_HIP(hipSetDevice(c->device));
  return upsample_launch(c, p, (const float4*)src, w, h, (const float4*)guide_full, (float4*)dst);
}

int pt_upsample(pt_context* c, const pt_upsample_params* params, const void* src, void* dst) {
  PT_SINGLE(c, "pt_upsample");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_upsample_params p;
  const int rp = upsample_params(params, &p);
  if (rp) return rp;
  const int rc = upsample_context_ok(c);
  if (rc) return rc;
  const int w = c->width, h = c->height;
  const int rs = upsample_size(w, h, p.scale);
  if (rs) return rs;
  const float4* in = src ? (const float4*)src : c->d_accum;
  const int ri = upsample_images_ok(in, nullptr, dst, w, h, p.scale, sizeof(float4));
  if (ri) return ri;
  PT_HIP(hipSetDevice(c->device));
  const int rg = upsample_guide(c, p.scale);
  if (rg) return rg;
  return upsample_launch(c, p, in, w, h, c->d_up_guide, (float4*)dst);
}

void* pt_upsampled_device_ptr(pt_context* c) {
  if (!c || c->group || !c->d_upsampled || c->upsampled_w == 0) return nullptr;
  return (void*)c->d_upsampled;
}

int pt_read_upsampled(pt_context* c, float* rgba, size_t n) {
  PT_SINGLE(c, "pt_read_upsampled");
  if (!c || !rgba) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_upsampled || c->upsampled_w == 0)
    return fail(PT_ERR_INVALID, "no library-owned upsampled image (pt_upsample or pt_upsample_images with a null destination)");
  return read_image(c, c->d_upsampled, c->upsampled_w, c->upsampled_h, 4, rgba, n);
}

void* pt_upsample_guide_device_ptr(pt_context* c) {
  if (!c || c->group || !up_guide_current(c, c->up_scale)) return nullptr;
  return (void*)c->d_up_guide;
}

int pt_upsample_info(pt_context* c, int info[8]) {
  PT_SINGLE(c, "pt_upsample_info");
  if (!c || !info) return fail(PT_ERR_INVALID, "null argument");
  const bool g = up_guide_current(c, c->up_scale);
  info[0] = g ? c->up_scale : 0;
  info[1] = g ? c->up_w * c->up_scale : 0;
  info[2] = g ? c->up_h * c->up_scale : 0;
  info[3] = c->up_guide_launches;
  info[4] = c->d_upsampled ? c->upsampled_w : 0;
  info[5] = c->d_upsampled ? c->upsampled_h : 0;
  info[6] = c->d_up_display ? c->up_display_w : 0;
  info[7] = c->d_up_display ? c->up_display_h : 0;
  return PT_OK;
}

int pt_upsample_display(pt_context* c, const pt_upsample_params* up_params, const pt_display_params* display_params,
                        const void* src, void* dst) {
  PT_SINGLE(c, "pt_upsample_display");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_upsample_params p;
  const int rp = upsample_params(up_params, &p);
  if (rp) return rp;
  pt_display_params dp;
  const int rd = display_checked_params(display_params, &dp);
  if (rd) return rd;
  const int rc = upsample_context_ok(c);
  if (rc) return rc;
  const int w = c->width, h = c->height;
  const int rs = upsample_size(w, h, p.scale);
  if (rs) return rs;
  const float4* in = src ? (const float4*)src : c->d_accum;
  const int ri = upsample_images_ok(in, nullptr, dst, w, h, p.scale, sizeof(uint32_t));
  if (ri) return ri;
  PT_HIP(hipSetDevice(c->device));
  const int rg = upsample_guide(c, p.scale);
  if (rg) return rg;
  const int W = w * p.scale, H = h * p.scale;
  uint32_t* out = (uint32_t*)dst;
  if (!out) {
    c->up_display_w = c->up_display_h = 0;
    const int ro = grow_dev(c, &c->d_up_display, &c->up_display_cap, (size_t)W * H);
    if (ro) return ro;
    out = c->d_up_display;
  }
  const int ro = order_shared(c);
  if (ro) return ro;
  const ptdp::MeterState* state = nullptr;
  if (dp.auto_exposure) {   // of the rendered pixels, not the upsampled ones
    const int rm = display_meter(c, dp, in, w, h);
    if (rm) return rm;
    state = (const ptdp::MeterState*)c->d_meter_state;
  }
  PT_HIP(ptd::launch_upsample_display(in, c->d_up_guide, out, w, h, p.scale, p.sigma_normal * p.sigma_normal,
                                      p.sigma_depth * p.sigma_depth, dp.tonemap, dp.exposure, dp.white * dp.white,
                                      state, c->stream));
  if (!dst) {
    c->up_display_w = W;
    c->up_display_h = H;
  }
  return mark_shared(c);
}

void* pt_display_upsampled_device_ptr(pt_context* c) {
  if (!c || c->group || !c->d_up_display || c->up_display_w == 0) return nullptr;
  return (void*)c->d_up_display;
}

int pt_read_display_upsampled(pt_context* c, unsigned char* rgba8, size_t n_bytes) {
  PT_SINGLE(c, "pt_read_display_upsampled");
  if (!c || !rgba8) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_up_display || c->up_display_w == 0)
    return fail(PT_ERR_INVALID, "no library-owned upsampled display image (pt_upsample_display with a null destination)");
  const size_t need = (size_t)c->up_display_w * c->up_display_h * 4;
  if (n_bytes < need) return fail(PT_ERR_INVALID, "output buffer too small: need " + std::to_string(need) + " bytes");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(hipMemcpyAsync(rgba8, c->d_up_display, need, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(hipStreamSynchronize(c->stream));
  return PT_OK;
}

}  // extern "C"
