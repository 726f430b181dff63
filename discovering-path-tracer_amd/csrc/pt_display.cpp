// pt_display.cpp — the display transform behind the C ABI (include/pathtracer.h):
// exposure, tone map and the 8-bit sRGB encode on the device, the metering pass
// of auto exposure, the 8-bit readback, and the host statement
// (pt_display_host, pt_display.h) beside them.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_display.h"

// Frees what this file allocates in a context (pt_destroy).
void display_release(pt_context* c) {
  dev_free(c->d_display);
  dev_free(c->d_meter_sum);
  dev_free(c->d_meter_n);
  if (c->d_meter_state) (void)hipFree(c->d_meter_state);
  c->d_meter_state = nullptr;
  for (auto& r : c->drb) {
    dev_free(r.dev);
    if (r.host) (void)hipHostFree(r.host);
    if (r.snap) (void)hipEventDestroy(r.snap);
    if (r.done) (void)hipEventDestroy(r.done);
  }
}

// Whether the metering state holds a previous scale: a metering call has run since it was last
// forgotten (display_forget).
static bool display_has_prev(const pt_context* c) { return c->meter_have && c->d_meter_state; }

static int display_params(const pt_display_params* in, pt_display_params* p) {
  if (in) *p = *in;
  else (void)pt_display_default_params(p);
  if (!ptdp::params_ok(p->tonemap, p->exposure, p->auto_exposure, p->key, p->white, p->adapt))
    return fail(PT_ERR_INVALID,
                "pt_display_params: tonemap 0-2, auto_exposure 0 or 1; exposure, key and white finite and > 0, "
                "white * white finite and non-zero; adapt in (0, 1]");
  return PT_OK;
}

int display_checked_params(const pt_display_params* in, pt_display_params* p) { return display_params(in, p); }

// The metering of a w x h source on the context's stream, behind order_shared: the scale lands in the
// state (c->d_meter_state), which the next metering call reads as the previous one.
int display_meter(pt_context* c, const pt_display_params& p, const float4* src, int w, int h) {
  const size_t tiles = (size_t)((w + 15) / 16) * (size_t)((h + 15) / 16);
  int rg = grow_dev(c, &c->d_meter_sum, &c->meter_cap[0], tiles);
  if (!rg) rg = grow_dev(c, &c->d_meter_n, &c->meter_cap[1], tiles);
  if (rg) return rg;
  if (!c->d_meter_state) PT_HIP(hipMalloc(&c->d_meter_state, sizeof(ptdp::MeterState)));
  PT_HIP(ptd::launch_display_meter(src, w, h, c->d_meter_sum, c->d_meter_n, p.key, p.adapt,
                                   display_has_prev(c) ? 1 : 0, (ptdp::MeterState*)c->d_meter_state, c->stream));
  c->meter_have = true;
  return PT_OK;
}

// The checks pt_display and pt_display_readback_begin share.
static int display_args(pt_context* c, const pt_display_params* params, const void* src, const void* dst,
                        pt_display_params* p) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  const int rp = display_params(params, p);
  if (rp) return rp;
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  if ((((uintptr_t)src) & 15) || (((uintptr_t)dst) & 3))
    return fail(PT_ERR_INVALID, "pt_display: the source must be 16-B aligned, the destination 4-B");
  const size_t n = (size_t)c->width * c->height;
  const char* s = src ? (const char*)src : (const char*)c->d_accum;
  if (dst && (const char*)dst < s + n * sizeof(float4) && s < (const char*)dst + n * sizeof(uint32_t))
    return fail(PT_ERR_INVALID, "pt_display: source and destination must not overlap");
  return PT_OK;
}

// The metering (if asked for) and the transform of checked images with validated params, on the
// context's stream.
static int display_launch(pt_context* c, const pt_display_params& p, const float4* src, uint32_t* out) {
  const int w = c->width, h = c->height;
  const ptdp::MeterState* state = nullptr;
  const int ro = order_shared(c);
  if (ro) return ro;
  if (p.auto_exposure) {
    const int rm = display_meter(c, p, src, w, h);
    if (rm) return rm;
    state = (const ptdp::MeterState*)c->d_meter_state;
  }
  PT_HIP(ptd::launch_display(src, out, (size_t)w * h, p.tonemap, p.exposure, p.white * p.white, state,
                             c->stream));
  return mark_shared(c);
}

extern "C" {

int pt_display_default_params(pt_display_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->tonemap = PT_TONEMAP_CLAMP;
  out->exposure = 1.0f;
  out->auto_exposure = 0;
  out->key = 0.18f;
  out->white = 4.0f;
  out->adapt = 1.0f;
  return PT_OK;
}

int pt_display_host(const float* rgba, int w, int h, const pt_display_params* params, float* auto_scale_io,
                    unsigned char* rgba8) {
  if (!rgba || !rgba8) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 31)) return fail(PT_ERR_INVALID, "bad resolution");
  pt_display_params p;
  const int rp = display_params(params, &p);
  if (rp) return rp;
  const size_t n = (size_t)w * (size_t)h;
  ptdp::Tone t = {p.tonemap, p.exposure, p.white * p.white};
  if (p.auto_exposure) {
    const float prev = auto_scale_io ? *auto_scale_io : 0.0f;
    if (!(prev == 0.0f || ptdp::pos_finite(prev)))
      return fail(PT_ERR_INVALID, "pt_display_host: the previous scale is 0 (none) or finite and > 0");
    const int bx = (w + 15) / 16, by = (h + 15) / 16;
    std::vector<float> partial((size_t)bx * by);
    uint32_t count = 0;
    for (int ty = 0; ty < by; ++ty)
      for (int tx = 0; tx < bx; ++tx) {
        float v[256];
        for (int i = 0; i < 256; ++i) {
          const int x = tx * 16 + (i & 15), y = ty * 16 + (i >> 4);
          bool metered = false;
          v[i] = 0.0f;
          if (x < w && y < h) {
            float4 c;
            memcpy(&c, rgba + 4 * ((size_t)y * w + x), sizeof c);
            v[i] = ptdp::meter_term(c, &metered);
          }
          count += metered ? 1u : 0u;
        }
        partial[(size_t)ty * bx + tx] = ptdp::tree256(v);
      }
    float lanes[256];
    for (int j = 0; j < 256; ++j) lanes[j] = ptdp::meter_lane(partial.data(), bx * by, j);
    const float scale = ptdp::meter_scale(ptdp::tree256(lanes), count, p.key, p.adapt, prev != 0.0f, prev);
    if (auto_scale_io) *auto_scale_io = scale;
    t.scale = p.exposure * scale;
  }
  for (size_t i = 0; i < n; ++i) {
    float4 c;
    memcpy(&c, rgba + 4 * i, sizeof c);
    const uint32_t word = ptdp::display_pixel(ptdp::kSrgb8T, c, t);
    rgba8[4 * i + 0] = (unsigned char)(word & 0xffu);
    rgba8[4 * i + 1] = (unsigned char)((word >> 8) & 0xffu);
    rgba8[4 * i + 2] = (unsigned char)((word >> 16) & 0xffu);
    rgba8[4 * i + 3] = (unsigned char)(word >> 24);
  }
  return PT_OK;
}

int pt_display(pt_context* c, const pt_display_params* params, const void* src, void* dst) {
  PT_SINGLE(c, "pt_display");
  pt_display_params p;
  const int ra = display_args(c, params, src, dst, &p);
  if (ra) return ra;
  PT_HIP(hipSetDevice(c->device));
  uint32_t* out = (uint32_t*)dst;
  if (!out) {
    c->display_w = c->display_h = 0;
    const int rd = grow_dev(c, &c->d_display, &c->display_cap, (size_t)c->width * c->height);
    if (rd) return rd;
    out = c->d_display;
  }
  const int rl = display_launch(c, p, src ? (const float4*)src : c->d_accum, out);
  if (rl) return rl;
  if (!dst) {
    c->display_w = c->width;
    c->display_h = c->height;
  }
  return PT_OK;
}

void* pt_display_device_ptr(pt_context* c) {
  if (!c || c->group || !c->d_display || c->display_w != c->width || c->display_h != c->height || c->display_w == 0)
    return nullptr;
  return (void*)c->d_display;
}

int pt_read_display(pt_context* c, unsigned char* rgba8, size_t n_bytes) {
  PT_SINGLE(c, "pt_read_display");
  if (!c || !rgba8) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_display || c->display_w == 0)
    return fail(PT_ERR_INVALID, "no library-owned display image (pt_display with a null destination)");
  const size_t need = (size_t)c->display_w * c->display_h * 4;
  if (n_bytes < need) return fail(PT_ERR_INVALID, "output buffer too small: need " + std::to_string(need) + " bytes");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(hipMemcpyAsync(rgba8, c->d_display, need, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(hipStreamSynchronize(c->stream));
  return PT_OK;
}

int pt_display_exposure(pt_context* c, float* auto_scale, uint32_t* n_metered) {
  PT_SINGLE(c, "pt_display_exposure");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  ptdp::MeterState s = {1.0f, 0u};
  if (display_has_prev(c)) {
    PT_HIP(hipSetDevice(c->device));
    const int ro = order_shared(c);
    if (ro) return ro;
    PT_HIP(hipMemcpyAsync(&s, c->d_meter_state, sizeof s, hipMemcpyDeviceToHost, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
  }
  if (auto_scale) *auto_scale = s.scale;
  if (n_metered) *n_metered = s.n;
  return PT_OK;
}

int pt_display_reset(pt_context* c) {
  PT_SINGLE(c, "pt_display_reset");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  display_forget(c);
  return PT_OK;
}

int pt_display_readback_begin(pt_context* c, const pt_display_params* params, const void* src, int* ticket) {
  PT_SINGLE(c, "pt_display_readback_begin");
  if (c && !ticket) return fail(PT_ERR_INVALID, "null argument");
  pt_display_params p;
  const int ra = display_args(c, params, src, nullptr, &p);
  if (ra) return ra;
  PT_HIP(hipSetDevice(c->device));
  if (!c->copy_stream) PT_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  // the free slot, else the older one (its unread result is dropped)
  const int slot = c->drb[0].ticket == 0 ? 0 : c->drb[1].ticket == 0 ? 1 : (c->drb[0].ticket < c->drb[1].ticket ? 0 : 1);
  pt_context::DisplayReadback& r = c->drb[slot];
  if (r.ticket) PT_HIP(hipEventSynchronize(r.done));
  r.ticket = 0;
  const size_t bytes = (size_t)c->width * c->height * sizeof(uint32_t);
  if (r.bytes != bytes) {
    { const int rc_ = quiesce(c); if (rc_) return rc_; }
    dev_free(r.dev);
    if (r.host) (void)hipHostFree(r.host);
    r.host = nullptr;
    r.bytes = 0;
    PT_HIP(hipMalloc((void**)&r.dev, bytes));
    PT_HIP(hipHostMalloc(&r.host, bytes, hipHostMallocDefault));
    r.bytes = bytes;
  }
  if (!r.snap) PT_HIP(hipEventCreateWithFlags(&r.snap, hipEventDisableTiming));
  if (!r.done) PT_HIP(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  const int rl = display_launch(c, p, src ? (const float4*)src : c->d_accum, r.dev);   // the snapshot
  if (rl) return rl;
  PT_HIP(hipEventRecord(r.snap, c->stream));
  PT_HIP(hipStreamWaitEvent(c->copy_stream, r.snap, 0));
  PT_HIP(hipMemcpyAsync(r.host, r.dev, bytes, hipMemcpyDeviceToHost, c->copy_stream));
  PT_HIP(hipEventRecord(r.done, c->copy_stream));
  r.w = c->width;
  r.h = c->height;
  r.ticket = c->drb_next_ticket++;
  *ticket = r.ticket;
  return PT_OK;
}

int pt_display_readback_end(pt_context* c, int ticket, unsigned char* rgba8, size_t n_bytes) {
  PT_SINGLE(c, "pt_display_readback_end");
  if (!c || !rgba8) return fail(PT_ERR_INVALID, "null argument");
  for (auto& r : c->drb) {
    if (r.ticket != ticket || ticket == 0) continue;
    const size_t need = (size_t)r.w * r.h * 4;
    if (n_bytes < need) return fail(PT_ERR_INVALID, "output buffer too small: need " + std::to_string(need) + " bytes");
    PT_HIP(hipSetDevice(c->device));
    PT_HIP(hipEventSynchronize(r.done));
    memcpy(rgba8, r.host, need);
    r.ticket = 0;
    return PT_OK;
  }
  return fail(PT_ERR_INVALID, "unknown or already collected readback ticket " + std::to_string(ticket));
}

}  // extern "C"
