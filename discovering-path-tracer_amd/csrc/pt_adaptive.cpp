// pt_adaptive.cpp — adaptive sampling behind the C ABI (include/pathtracer.h):
// the stopping rule on the host and on the caller's device images
// (pt_adaptive_select_host, pt_adaptive_select; the statement is pt_denoise.h's
// adaptive_error / adaptive_next), the rounds of an adaptive render
// (pt_adaptive_begin, pt_adaptive_advance: rule, live list, one launch of
// kernels/adaptive.h per round, or with PT_OPT_ADAPTIVE_WF a round of the
// wavefront pipeline, kernels/wf_adaptive.h; nothing waited for), its reads, and the
// variance-guided filter of its result (pt_adaptive_denoise).  What the calls
// refuse and which kernel they run is pt_plan.h's plan_adaptive.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_denoise.h"
#include "pt_plan.h"

void adaptive_release(pt_context* c) {
  dev_free(c->d_ad_counts);
  dev_free(c->d_ad_added);
  dev_free(c->d_ad_errors);
  dev_free(c->d_ad_list);
  dev_free(c->d_ad_live);
  dev_free(c->d_ad_var);
}

static ptdn::AdaptiveParams statement_params(const pt_adaptive_params& p) {
  return {p.min_batches, p.max_batches, p.step, p.threshold, p.lum_floor};
}

static int tiles_of(int w, int h) { return ((w + 15) / 16) * ((h + 15) / 16); }

// One round's launch at `spl` lanes over the list the stream has just been given.  round: 0 = pt_adaptive_begin's,
// k = the k-th of pt_adaptive_advance.  The path-recursive kernel takes the batches from the list's entries; a
// wavefront round (ap.wf) takes them from the host, which knows them without reading the list: every tile starts at
// min_batches, a tile is live only if it was live in every earlier round, and a live tile advances by
// min(step, max - n), so all live entries of round k >= 1 hold {min + (k - 1) * step, min(step, max - that)}.
static int launch_round(pt_context* c, const AdaptivePlan& ap, const pt_adaptive_params& a, uint32_t round, int spl) {
  ptd::RenderParams p{};
  const int rp = adaptive_render_params(c, ap, spl, &p);
  if (rp) return rp;
  if (ap.wf) {
    p.first_batch = round == 0 ? 0u : a.min_batches + (round - 1u) * a.step;   // < max_batches: the round exists
    p.n_batches = round == 0 ? a.min_batches : std::min(a.step, a.max_batches - p.first_batch);
    return adaptive_launch_wavefront(c, ap, std::max(a.min_batches, std::min(a.step, a.max_batches)), &p);
  }
  PT_HIP(ptd::launch_render_adaptive(p, ap.lds, c->d_ad_list, c->d_ad_live, c->stream));
  return PT_OK;
}

// Waits for the enqueued rounds and copies `n` elements of a state array.
template <class T>
static int read_state(pt_context* c, const T* dev, T* out, size_t n) {
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(hipMemcpyAsync(out, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  PT_HIP(hipStreamSynchronize(c->stream));
  return PT_OK;
}

extern "C" {

int pt_adaptive_default_params(pt_adaptive_params* out) {
  if (!out) return fail(PT_ERR_INVALID, "null argument");
  out->min_batches = 4;
  out->max_batches = 64;
  out->step = 15;   // 4, 19, 34, 49, 64: four rounds (a round's fixed cost and its thin launch favour few)
  out->threshold = 0.09f;
  out->lum_floor = 2.0f;
  return PT_OK;
}

static int adaptive_params(const pt_adaptive_params* in, pt_adaptive_params* p) {
  if (in)
    *p = *in;
  else
    (void)pt_adaptive_default_params(p);
  if (!ptdn::adaptive_params_ok(p->min_batches, p->max_batches, p->step, p->threshold, p->lum_floor))
    return fail(PT_ERR_INVALID, kAdaptiveBadParams);
  return PT_OK;
}

int pt_adaptive_select_host(const float* moments, const uint32_t* counts, int w, int h, const pt_adaptive_params* params,
                            uint32_t* next_counts, float* errors) {
  if (!moments || !counts || !next_counts) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 31)) return fail(PT_ERR_INVALID, "bad resolution");
  pt_adaptive_params p;
  const int rp = adaptive_params(params, &p);
  if (rp) return rp;
  ptdn::adaptive_select_image(moments, counts, w, h, statement_params(p), next_counts, errors);
  return PT_OK;
}

int pt_adaptive_select(pt_context* c, const void* moments, const void* counts, int w, int h,
                       const pt_adaptive_params* params, void* next_counts, void* errors) {
  PT_SINGLE(c, "pt_adaptive_select");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!moments || !counts || !next_counts || !errors) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 31)) return fail(PT_ERR_INVALID, "bad resolution");
  pt_adaptive_params p;
  const int rp = adaptive_params(params, &p);
  if (rp) return rp;
  if (((uintptr_t)moments & 7) || (((uintptr_t)counts | (uintptr_t)next_counts | (uintptr_t)errors) & 3))
    return fail(PT_ERR_INVALID, "pt_adaptive_select: moments must be 8-B aligned, counts, next_counts and errors 4-B");
  if (errors == counts || errors == next_counts || moments == next_counts || moments == errors)
    return fail(PT_ERR_INVALID, "pt_adaptive_select: an output is also an input (only next_counts may be counts)");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_adaptive_select((const float2*)moments, (const uint32_t*)counts, w, h, statement_params(p),
                                     (uint32_t*)next_counts, (float*)errors, nullptr, c->stream));
  accum_overwritten(c, next_counts);
  accum_overwritten(c, errors);
  return mark_shared(c);
}

int pt_adaptive_begin(pt_context* c, const pt_adaptive_params* params) {
  PT_SINGLE(c, "pt_adaptive_begin");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_adaptive_params p;
  const int rp = adaptive_params(params, &p);
  if (rp) return rp;
  const AdaptivePlan ap = plan_adaptive(*c, p);
  if (ap.refuse) return fail(ap.refuse_code, std::string("pt_adaptive_begin: ") + ap.refuse);
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (!c->has_camera) return fail(PT_ERR_INVALID, "no camera set");
  if (c->n_lights < 1) return fail(PT_ERR_INVALID, "no lights uploaded");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  PT_HIP(hipSetDevice(c->device));
  const int tiles = tiles_of(c->width, c->height);
  const size_t npx = (size_t)c->width * c->height;
  int rc = grow_dev(c, &c->d_ad_counts, &c->ad_cap[0], (size_t)tiles);
  if (!rc) rc = grow_dev(c, &c->d_ad_added, &c->ad_cap[1], (size_t)tiles);
  if (!rc) rc = grow_dev(c, &c->d_ad_errors, &c->ad_cap[2], (size_t)tiles);
  if (!rc) rc = grow_dev(c, &c->d_ad_list, &c->ad_cap[3], (size_t)tiles);
  if (!rc && !c->d_ad_live) PT_HIP(hipMalloc((void**)&c->d_ad_live, sizeof(int)));
  if (!rc && (!c->d_moments || c->moments_cap < npx)) rc = grow_dev(c, &c->d_moments, &c->moments_cap, npx);
  if (rc) return rc;
  rc = pt_clear_accum(c);   // +0 everywhere, the moments with it; ends an earlier adaptive render
  if (rc) return rc;
  c->culled_state = 0;      // the rounds write the image without the bookkeeping of the culled items
  // round 0: every tile listed with batches 0..min-1, the errors 0 until a rule has run
  PT_HIP(hipMemsetAsync(c->d_ad_errors, 0, (size_t)tiles * sizeof(float), c->stream));
  PT_HIP(ptd::launch_adaptive_fill(c->d_ad_counts, c->d_ad_added, tiles, p.min_batches, c->stream));
  PT_HIP(ptd::launch_adaptive_compact(c->d_ad_counts, c->d_ad_added, c->width, c->height, c->d_ad_list, c->d_ad_live,
                                      c->stream));
  rc = launch_round(c, ap, p, 0, ap.spl0);
  if (rc) return rc;
  c->last_kernel = ap.wf ? 3 : 1;
  c->ad_params = p;
  c->ad_rounds = ap.rounds;
  c->ad_rounds_done = 0;
  c->ad_tiles = tiles;
  c->ad_active = true;
  return mark_shared(c);
}

int pt_adaptive_advance(pt_context* c, uint32_t rounds) {
  PT_SINGLE(c, "pt_adaptive_advance");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->ad_active) return fail(PT_ERR_INVALID, "pt_adaptive_advance: no adaptive render in progress (pt_adaptive_begin)");
  // the options may have changed since the rounds began: the plan is made again (every kernel gives the same bits)
  const AdaptivePlan ap = plan_adaptive(*c, c->ad_params);
  if (ap.refuse) return fail(ap.refuse_code, std::string("pt_adaptive_advance: ") + ap.refuse);
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  const ptdn::AdaptiveParams a = statement_params(c->ad_params);
  for (uint32_t r = 0; r < rounds && c->ad_rounds_done < c->ad_rounds; ++r) {
    PT_HIP(ptd::launch_adaptive_select(c->d_moments, c->d_ad_counts, c->width, c->height, a, c->d_ad_counts,
                                       c->d_ad_errors, c->d_ad_added, c->stream));
    PT_HIP(ptd::launch_adaptive_compact(c->d_ad_counts, c->d_ad_added, c->width, c->height, c->d_ad_list,
                                        c->d_ad_live, c->stream));
    const int rc = launch_round(c, ap, c->ad_params, c->ad_rounds_done + 1u, ap.spl);
    if (rc) return rc;
    c->ad_rounds_done++;
    c->ad_var_valid = false;
  }
  return mark_shared(c);
}

static int adaptive_ready(pt_context* c, const char* name) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->ad_active) return fail(PT_ERR_INVALID, std::string(name) + ": no adaptive render (pt_adaptive_begin)");
  return PT_OK;
}

int pt_adaptive_info(pt_context* c, uint32_t* rounds_done, uint32_t* live_tiles, unsigned long long* samples_total) {
  PT_SINGLE(c, "pt_adaptive_info");
  const int ra = adaptive_ready(c, "pt_adaptive_info");
  if (ra) return ra;
  std::vector<uint32_t> counts((size_t)c->ad_tiles);
  int live = 0;
  int rc = read_state(c, c->d_ad_counts, counts.data(), counts.size());
  if (!rc) rc = read_state(c, c->d_ad_live, &live, 1);
  if (rc) return rc;
  if (rounds_done) *rounds_done = c->ad_rounds_done;
  if (live_tiles) *live_tiles = c->ad_rounds_done >= c->ad_rounds ? 0u : (uint32_t)live;
  if (samples_total) {
    const int bx = (c->width + 15) / 16;
    unsigned long long s = 0;
    for (int b = 0; b < c->ad_tiles; ++b) {
      const int tw = std::min(16, c->width - (b % bx) * 16), th = std::min(16, c->height - (b / bx) * 16);
      s += (unsigned long long)counts[(size_t)b] * (unsigned long long)(tw * th);
    }
    *samples_total = s;
  }
  return PT_OK;
}

int pt_adaptive_read_counts(pt_context* c, uint32_t* counts, float* errors, size_t n_tiles) {
  PT_SINGLE(c, "pt_adaptive_read_counts");
  const int ra = adaptive_ready(c, "pt_adaptive_read_counts");
  if (ra) return ra;
  if (n_tiles != (size_t)c->ad_tiles)
    return fail(PT_ERR_INVALID, "pt_adaptive_read_counts: the frame has " + std::to_string(c->ad_tiles) + " tiles");
  int rc = PT_OK;
  if (counts) rc = read_state(c, c->d_ad_counts, counts, n_tiles);
  if (!rc && errors) rc = read_state(c, c->d_ad_errors, errors, n_tiles);
  return rc;
}

int pt_adaptive_read_live(pt_context* c, int* entries, size_t max_entries, uint32_t* n_live) {
  PT_SINGLE(c, "pt_adaptive_read_live");
  const int ra = adaptive_ready(c, "pt_adaptive_read_live");
  if (ra) return ra;
  if (!n_live) return fail(PT_ERR_INVALID, "null argument");
  int live = 0;
  int rc = read_state(c, c->d_ad_live, &live, 1);
  if (rc) return rc;
  if (live < 0 || live > c->ad_tiles) return fail(PT_ERR_HIP, "pt_adaptive_read_live: the live count is out of range");
  *n_live = (uint32_t)live;
  const size_t n = std::min((size_t)live, max_entries);
  if (entries && n > 0) rc = read_state(c, (const int*)c->d_ad_list, entries, 4 * n);
  return rc;
}

void* pt_adaptive_device_ptr(pt_context* c, int which) {
  if (!c || c->group || !c->ad_active) return nullptr;
  return which == 0 ? (void*)c->d_ad_counts : which == 1 ? (void*)c->d_ad_errors
         : which == 2 && c->ad_var_valid ? (void*)c->d_ad_var : nullptr;
}

int pt_adaptive_denoise(pt_context* c, const pt_denoise_var_params* params, void* dst) {
  PT_SINGLE(c, "pt_adaptive_denoise");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  pt_denoise_var_params p;
  const int rp = post_denoise_var_params(params, &p);
  if (rp) return rp;
  const int ra = adaptive_ready(c, "pt_adaptive_denoise");
  if (ra) return ra;
  if (((uintptr_t)dst) & 15) return fail(PT_ERR_INVALID, "images must be 16-B aligned");
  if (dst && (float4*)dst == c->d_accum) return fail(PT_ERR_INVALID, "pt_adaptive_denoise: source and destination must differ");
  PT_HIP(hipSetDevice(c->device));
  if (!c->guide_valid) {
    const int rg = pt_render_guide(c);
    if (rg) return rg;
  }
  const int rv = grow_dev(c, &c->d_ad_var, &c->ad_var_cap, (size_t)c->width * c->height);
  if (rv) return rv;
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_adaptive_var(c->d_moments, c->d_ad_counts, c->d_ad_var, c->width, c->height, c->stream));
  c->ad_var_valid = true;
  const int rm = mark_shared(c);
  if (rm) return rm;
  return post_var_filter(c, p, c->d_accum, c->d_ad_var, c->d_guide, (float4*)dst);
}

}  // extern "C"
