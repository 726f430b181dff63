// pt_context.h — internal: the context behind the C ABI (include/pathtracer.h)
// and the helpers the shim's translation units share.  pt_api.cpp is the core
// (create/destroy, uploads, item lists, render_impl and its steps, options,
// exchange, stats, timing); pt_plan.h the launch plan, every policy render_impl
// carries out, as one pure function (plan_launch); pt_post.cpp the
// post-processing chain (guide, filters, temporal accumulation);
// pt_adaptive.cpp adaptive sampling; pt_display.cpp the display transform; pt_upsample.cpp
// guide-driven upsampling; pt_rays.cpp the batched ray queries; pt_dist.cpp
// the RCCL step loop; pt_group.cpp the multi-device context.  The fields of
// pt_context are grouped in that order.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pathtracer.h"
#include "pt_device.h"
#include "pt_group.h"

// Internal to the library: none of this enters its dynamic symbol table.
#pragma GCC visibility push(hidden)

// Sets pt_last_error() on the calling thread and returns code.
inline int fail(int code, const std::string& msg) { return pt_fail_internal(code, msg); }

#define PT_HIP(call)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) return fail(PT_ERR_HIP, std::string(#call ": ") + hipGetErrorString(e_)); \
  } while (0)

// The calls a multi-device context (pt_create_multi) refuses.
#define PT_SINGLE(c, name)                                                                              \
  do {                                                                                                  \
    if ((c) && (c)->group) return fail(PT_ERR_UNSUPPORTED, name ": not on a multi-device context (pt_create_multi)"); \
  } while (0)

template <class T>
void dev_free(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

struct DistState;   // pt_dist.cpp

struct pt_context {
  // ---- pt_api.cpp: device, streams and the order of work across them ----------
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // Launches that write context-owned buffers (the accumulation buffer, the
  // wavefront path buffers) are ordered across streams: the next such launch
  // waits for the last one when it runs on another stream (order_shared).
  hipEvent_t shared_ev = nullptr;
  hipStream_t shared_stream = nullptr;
  // Every stream this context has enqueued work on that reads its buffers
  // (node/triangle arrays, item tables, accumulation and wavefront buffers),
  // with an event recorded after the last such work (note_use).  A host-side
  // rebuild of those buffers waits on these events only (quiesce), never on
  // the whole device, so it does not wait on another component's RCCL or
  // torch work sharing the GPU.
  struct Use {
    hipStream_t stream;
    hipEvent_t ev;
  };
  std::vector<Use> uses;

  // ---- pt_api.cpp: scene, lights, camera, frame (the uploads) -----------------
  float4* d_nodes = nullptr;        // threaded, implied internal nodes collapsed (fast kernel)
  int n_nodes = 0;
  float4* d_nodes_full = nullptr;   // threaded, every reference node (stats mode)
  int n_nodes_full = 0;
  float4* d_sweep = nullptr;        // the sweep table of a tiny scene (scene/small_sweep.h), or null
  float4* d_sweep_plain = nullptr;  // ... and the same table without hull codes (PT_OPT_SWEEP_HULL 0)
  int sweep_boxes = 0, sweep_leaves = 0;
  int sweep_hull = 0;               // boxes of the table with a hull code
  // the cube table (scene/small_sweep.h SmallSweep::cube, its box 0 bitwise root_lo / root_hi below): the
  // faces' under words and the root's, as the SWEEP 3 kernels take them (PT_OPT_SWEEP_CUBE)
  bool sweep_cube = false;
  uint32_t cube_under[6] = {0, 0, 0, 0, 0, 0};
  uint32_t cube_all = 0;
  // culled wide walk (wide_walk.h): nodes, triangle records by rank, rank ->
  // slot, per-lane stack overflow areas (grown on demand)
  float4* d_wide = nullptr;
  float4* d_wide_q = nullptr;        // the same wide nodes in the 64-B layout
  float4* d_wide_leafbox = nullptr;  // the reference's leaf boxes by rank (64-B walk)
  float4* d_wide_tris = nullptr;
  int* d_wide_rank_of = nullptr;
  int2* d_wide_ovf = nullptr;
  long long wide_ovf_lanes = 0;
  int wide_ovf_stack = 0;   // the stack bound d_wide_ovf was sized for
  int n_wide = 0, wide_stack = 0;
  std::string wide_reason = "no scene";
  float4* d_tris = nullptr;
  int n_tris = 0;
  float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};   // root AABB of the uploaded tree
  bool exit_normals = false;   // some triangle's stored normal is axis-pure (pt_isect.h exit_normal)
  bool has_scene = false;
  ptd::LightRec* d_lights = nullptr;
  ptd::LightDev* d_lights_dev = nullptr;
  int n_lights = 0;
  std::vector<pt_area_light> lights_host;
  int scene_serial = 0;                        // bumped by scene and light uploads
  float cam[16] = {0};
  bool has_camera = false;
  pt_params params{4, 3};
  float4* d_accum = nullptr;
  bool own_accum = false;
  int width = 0, height = 0;

  // ---- pt_api.cpp: options (pt_set_option) -------------------------------------
  int opt_kernel = 0;         // PT_OPT_KERNEL: 0 auto, 1 path-recursive, 3 wavefront
  int opt_scene_lds = 1;      // PT_OPT_SCENE_IN_LDS: 0 never, 1 auto, 2 always
  int opt_sample_lanes = 0;   // PT_OPT_SAMPLE_LANES: 0 auto, else 1/2/4/8
  int opt_fresh = 0;          // PT_OPT_FRESH_BATCH0
  int opt_item_order = -1;    // PT_OPT_ITEM_ORDER (-1 auto)
  int opt_mixed = -1;         // PT_OPT_MIXED_LANES: -1 auto, 0 off, k = whole tiles for k % of the resident slots
  int opt_cull = 1;           // PT_OPT_PRIMARY_CULL
  int opt_cull_tight = 1;     // PT_OPT_CULL_TIGHT
  int opt_cull_foot = -1;     // PT_OPT_CULL_FOOTPRINT: -1 on unless counting, 0 off, 1 on
  int opt_count = 0;          // PT_OPT_COUNT_TRACED
  int opt_small_sweep = -1;   // PT_OPT_SMALL_SWEEP: -1 auto (kSweepAutoBoxes), 0 off, 1 whenever the scene has a table
  int opt_sweep_hull = 1;     // PT_OPT_SWEEP_HULL
  int opt_sweep_cube = 1;     // PT_OPT_SWEEP_CUBE
  int opt_exit_skip = 1;      // PT_OPT_EXIT_SKIP
  int opt_wide = 1;           // PT_OPT_WIDE
  int opt_wide_node = 64;     // PT_OPT_WIDE_NODE
  int opt_wide_build = 1;     // PT_OPT_WIDE_BUILD (pt::WideBuild; read at upload)
  int opt_wf_fuse = 1;        // PT_OPT_WF_FUSE
  int opt_wf_tail = -1;       // PT_OPT_WF_TAIL (-1 auto)
  int opt_wf_grid = 100;      // PT_OPT_WF_GRID (percent of a full-occupancy traversal grid)
  int opt_wf_refill = 0;      // PT_OPT_WF_REFILL (0 auto)
  int opt_wf_paths = 0;       // PT_OPT_WF_PATHS (0 = 2^27)
  int opt_wf_streams = 1;     // PT_OPT_WF_STREAMS (2 measured slower: 10M cloud +9 %, sphere -0.8 %)
  int opt_timing = 0;         // PT_OPT_LAUNCH_TIMING: event pair on every k-th launch, 0 = none (default:
                              // a pair costs the one-stream frame ~10 us, profiles/r06a)
  int opt_denoise_lds = 1;    // PT_OPT_DENOISE_LDS
  int opt_moments = 0;        // PT_OPT_MOMENTS
  uint32_t opt_seed_base = 0; // PT_OPT_SEED_BASE
  int opt_adaptive_wf = 0;    // PT_OPT_ADAPTIVE_WF: adaptive rounds on the wavefront pipeline
  int opt_rays_refill = 1;    // PT_OPT_RAYS_REFILL: pt_trace_rays' wide walk refills lanes from a ray counter
  bool stats_mode = false;    // pt_set_stats_mode

  // ---- pt_api.cpp: partition and item lists -------------------------------------
  int nranks = 1, rank = 0;
  std::vector<int> slots{1};    // partition slots per rank (pt_set_partition_slots)
  std::vector<ptd::Part> parts;  // every rank's share, derived from slots (ensure_parts)
  bool parts_valid = false;     // parts match slots
  bool parts_synced = false;    // d_parts holds parts
  int* d_parts = nullptr;       // every rank's slot positions, kMaxSlots ints each (rank_tile)
  size_t parts_cap = 0;
  std::vector<int> parts_key;
  // compact-launch item lists (live items, then culled ones), rebuilt when
  // the frame, partition, sample lanes or cull rectangles change
  int* d_items = nullptr;
  size_t items_cap = 0;
  int n_live_items = 0, n_culled_items = 0;   // launched live items (mixed lanes: whole tiles + parts)
  bool items_mixed = false;                    // the live origins carry per-item lane counts
  std::vector<int> block_lanes;                // lanes per 16x16 block in the current item lists (0: not launched)
  size_t culled_org_off = 0;   // h_items / d_items: where the culled items' first pixels start
  size_t live_org_off = 0;     // ... and the live items' ones
  std::vector<int> h_items;
  std::vector<float> items_key;
  std::vector<float> items_scratch;   // the per-launch key, built without reallocating
  // the footprint table the kernels read (PT_OPT_CULL_FOOTPRINT, RenderParams::foot) and the host's copy of
  // what it holds: kMaxCullRects footprints, then as many sure regions, of 16 floats each (pt_cull.h
  // kFootprintFloats, which this header does not include; pt_api.cpp asserts the size)
  float* d_foot = nullptr;
  float foot_up[2 * ptd::kMaxCullRects * 16] = {};

  // ---- pt_api.cpp: the mixed-lane scheduler (mix_feedback) ------------------------
  unsigned* d_cost = nullptr;                  // per 16x4 part: summed wave durations of a measuring launch
  unsigned* h_cost = nullptr;                  // pinned copy
  size_t cost_n = 0;                           // blocks allocated
  hipEvent_t cost_ev = nullptr;
  bool cost_pending = false, cost_stale = false, cost_measure = false, cost_ready = false;
  int cost_stable = 0, cost_frames = 0, cost_gen = 0;
  std::vector<float> cost_key, cost_scratch;
  std::vector<int> cost_lanes;                 // block_lanes of the measuring launch
  std::vector<double> block_cost;              // per 16x4 part, at one lane per pixel (averaged)
  int last_mix = 0;                            // pt_mixed_info: the last launch's schedule
  long long render_slots = -1;                 // resident LDS render workgroups (mixed lanes' budget)
  size_t render_slots_lds = 0;                 // ... at this many bytes of staged scene
  bool render_slots_sweep = false;             // ... of the sweep-walk kernel (false: the threaded walk's)

  // ---- pt_api.cpp: render_impl's launches ------------------------------------------
  ptd::RenderParams last{};     // configuration of the last pt_render
  bool last_valid = false;
  int last_kernel = 0;        // kernel of the last render (1 recursive, 3 wavefront)
  // What the accumulation buffer's culled items hold (culled_before, culled_after): 0 not
  // known, 1 finite (+-0 after a clear), 2 (0,0,0,1) in every culled item of
  // the item layout culled_key in buffer culled_buf.  Only the library's own
  // calls are assumed to write the buffer (accum_overwritten).
  int culled_state = 0;
  std::vector<float> culled_key;
  const void* culled_buf = nullptr;
  // per-pixel luminance moments (PT_OPT_MOMENTS), folded by the render launches
  float2* d_moments = nullptr;         // W x H {m1, m2}
  size_t moments_cap = 0;              // pixels d_moments holds
  bool moments_valid = false;          // d_moments holds batches 0..moments_n-1 of the current frame
  uint32_t moments_n = 0;
  uint32_t seed_extra = 0;             // inside pt_temporal_advance: the samples rendered since the last reset
  // wavefront pipeline buffers (PT_OPT_KERNEL 3), grown on demand
  ptd::WfBuffers wf{};
  void* wf_block = nullptr;
  long long wf_fail = 0;      // wavefront paths whose allocation failed (0: none)
  hipStream_t wf_stream2 = nullptr;           // the wavefront pipeline's second half (created on first use)
  hipEvent_t wf_fork = nullptr, wf_join = nullptr;

  // ---- pt_api.cpp: sparse exchange (this rank's live items, and all ranks' on the root)
  int* d_pack_items = nullptr;
  size_t pack_cap = 0;
  int n_pack_items = 0;
  std::vector<float> pack_key;
  int* d_unpack = nullptr;      // per entry: rank, x0, y0, slot (-1 = culled)
  size_t unpack_cap = 0;
  int n_unpack = 0;
  int* d_unpack_live = nullptr;   // the same table without the culled items' entries
  size_t unpack_live_cap = 0;
  int n_unpack_live = 0;
  std::vector<float> unpack_key;
  std::vector<float> packed_key;   // frame parameters of the last pt_render_packed
  std::vector<float> key_scratch;  // per-launch frame key, built without reallocating

  // ---- pt_api.cpp: progressive loop, readback, stats, timing ------------------------
  // progressive loop (VulkanRayTracer::mainLoop, :717-865)
  float prog_cam[16] = {0};
  bool prog_has_cam = false;
  uint32_t prog_batch = 0;
  // double-buffered asynchronous readback: device snapshot -> pinned host
  struct Readback {
    float4* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    hipEvent_t snap = nullptr, done = nullptr;
    int ticket = 0;        // 0 = free
    int w = 0, h = 0;
  } rb[2];
  hipStream_t copy_stream = nullptr;
  int rb_next_ticket = 1;
  unsigned long long* d_stats = nullptr;
  bool timed = false;
  // ring of event pairs, one per render launch since pt_reset_launch_times
  static constexpr int kRing = 512;
  hipEvent_t ring[kRing][2] = {};
  int ring_n = 0;
  int last_slot = 0;          // ring slot of the newest launch (pt_last_launch_ms)
  long long launch_n = 0;     // render launches since pt_reset_launch_times
  long long ring_launch[kRing] = {};   // launch number of each recorded pair

  // ---- pt_post.cpp: guide image, filters, temporal accumulation (freed by post_release)
  // first-hit guide image and a-trous filter (pt_render_guide, pt_denoise):
  // library-owned W x H float4 images, grown on demand
  float4* d_guide = nullptr;
  size_t guide_cap = 0;                // pixels d_guide holds
  bool guide_valid = false;            // d_guide is the guide of the current scene, camera and size
  float4* d_dn_scratch[2] = {nullptr, nullptr};   // the passes' ping-pong images
  size_t dn_scratch_cap[2] = {0, 0};
  float4* d_denoised = nullptr;        // pt_denoise's destination when the caller gives none
  size_t denoised_cap = 0;
  int denoised_w = 0, denoised_h = 0;  // size of the image d_denoised holds (0: none yet)
  float* d_var[2] = {nullptr, nullptr};   // pt_denoise_var's variance planes
  size_t var_cap[2] = {0, 0};
  // temporal accumulation (pt_temporal_advance)
  struct TemporalSet {                 // one of the two library-owned result sets
    float4* color = nullptr;
    float2* moments = nullptr;
    float* length = nullptr;
    float* variance = nullptr;
    size_t cap = 0;                    // pixels each image holds
  } tset[2];
  int t_cur = 0;                       // the set the last pt_temporal_advance wrote
  uint32_t t_frames = 0, t_samples = 0;   // since the last reset; t_frames 0: no history
  float t_cam[16] = {0};               // the last frame's camera
  int t_w = 0, t_h = 0;                // ... and size
  // the last frame's guide: d_guide while no later pt_render_guide has run (guide_serial ==
  // t_guide_serial), else d_guide_prev, where that pt_render_guide put it aside
  float4* d_guide_prev = nullptr;
  size_t guide_prev_cap = 0;
  unsigned long long guide_serial = 0, t_guide_serial = 0;
  bool t_guide_aside = false;
  float* d_spatial_var = nullptr;      // pt_temporal_denoise_spatial's variance plane
  size_t spatial_var_cap = 0;

  // ---- pt_adaptive.cpp: adaptive sampling (freed by adaptive_release) ---------------------
  bool ad_active = false;              // between pt_adaptive_begin and what ends the state (adaptive_forget)
  pt_adaptive_params ad_params{};
  uint32_t ad_rounds_done = 0, ad_rounds = 0;   // rounds enqueued since begin; rounds that can change a count
  int ad_tiles = 0;                    // tiles of the frame the state was begun on
  uint32_t* d_ad_counts = nullptr;     // per tile (raster order): n_T once the enqueued rounds have run
  uint32_t* d_ad_added = nullptr;      // ... and the batches the last round added (0: not live)
  float* d_ad_errors = nullptr;        // ... and E_T of the last round's rule
  int4* d_ad_list = nullptr;           // the last round's live list
  size_t ad_cap[4] = {0, 0, 0, 0};     // tiles the four hold
  int* d_ad_live = nullptr;            // the list's length
  float* d_ad_var = nullptr;           // pt_adaptive_denoise's variance plane
  size_t ad_var_cap = 0;
  bool ad_var_valid = false;

  // ---- pt_display.cpp: the display transform (freed by display_release) -------------------
  uint32_t* d_display = nullptr;       // pt_display's destination when the caller gives none: RGBA8 words
  size_t display_cap = 0;
  int display_w = 0, display_h = 0;    // size of the image d_display holds (0: none yet)
  float* d_meter_sum = nullptr;        // the metering's partial per 16x16 tile: the sum of the terms
  uint32_t* d_meter_n = nullptr;       // ... and the metered pixels
  size_t meter_cap[2] = {0, 0};
  void* d_meter_state = nullptr;       // ptdp::MeterState: the scale the last metering call used, its count
  bool meter_have = false;             // ... and holds one: the next metering call has a previous scale
  struct DisplayReadback {             // pt_display_readback_begin/end: as Readback, 4 B a pixel
    uint32_t* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    hipEvent_t snap = nullptr, done = nullptr;
    int ticket = 0;                    // 0 = free
    int w = 0, h = 0;
  } drb[2];
  int drb_next_ticket = 1;

  // ---- pt_upsample.cpp: guide-driven upsampling (freed by upsample_release) ----------------
  // the guide of the full frame, (up_scale * width) x (up_scale * height), kept until the scene, the camera,
  // the frame size or the scale changes
  float4* d_up_guide = nullptr;
  size_t up_guide_cap = 0;
  int up_scale = 0;                    // the scale d_up_guide was rendered for (0: it holds no guide)
  int up_w = 0, up_h = 0;              // ... and the render size
  float up_cam[16] = {0};              // ... and the camera
  int up_guide_launches = 0;           // guide launches of pt_upsample and pt_upsample_display so far
  float4* d_upsampled = nullptr;       // pt_upsample's destination when the caller gives none
  size_t upsampled_cap = 0;
  int upsampled_w = 0, upsampled_h = 0;   // full size of the image d_upsampled holds (0: none yet)
  uint32_t* d_up_display = nullptr;    // pt_upsample_display's destination when the caller gives none
  size_t up_display_cap = 0;
  int up_display_w = 0, up_display_h = 0;

  // ---- pt_rays.cpp: batched ray queries (freed by rays_release) ---------------------------
  uint32_t* d_rays_counters = nullptr; // the wide kernel's ray cursor and its count of marked rays
  int* d_rays_slot = nullptr;          // rank -> triangle index of the scene's wide tree, built by the first
  size_t rays_slot_cap = 0;            // query after an upload (rays_slot_serial == scene_serial: current)
  int rays_slot_serial = -1;
  void* d_rays_in = nullptr;           // pt_trace_rays_sync's staging buffers, grown on demand
  void* d_rays_out = nullptr;
  size_t rays_in_cap = 0, rays_out_cap = 0;   // rays / answers of 32 B they hold

  // ---- pt_radiance.cpp: radiance queries (freed by radiance_release) ------------------------
  int opt_radiance_chunk = 0;          // PT_OPT_RADIANCE_CHUNK: paths per chunk, 0 auto (kRadianceAutoChunk)
  float4* d_rad_colors = nullptr;      // the path-recursive kernel's colour per path of a chunk, grown on demand
  size_t rad_colors_cap = 0;           // (the wavefront pipeline's are wf.colors)
  void* d_rad_in = nullptr;            // pt_trace_radiance_sync's staging buffers, grown on demand
  float4* d_rad_out = nullptr;
  size_t rad_in_cap = 0, rad_out_cap = 0;   // queries of 32 B / answers of 16 B they hold

  // ---- pt_dist.cpp, pt_group.cpp ------------------------------------------------------
  DistState* dist = nullptr;          // pt_dist_init
  bool in_dist = false;                // inside pt_dist_run: it records the use events itself
  pt_group* group = nullptr;           // pt_create_multi: every call goes to the group (pt_group.cpp)
};

// The temporal history is forgotten (pt_temporal_reset; a new scene, lights, params, frame size or
// bound buffer): the next pt_temporal_advance runs without history and seeds from the seed base again.
inline void temporal_forget(pt_context* c) {
  c->t_frames = 0;
  c->t_samples = 0;
  c->t_guide_aside = false;
}

// The metering state of the display transform is forgotten (pt_display_reset; a new scene, frame size or
// bound buffer): the next metering pt_display runs without a previous scale.
inline void display_forget(pt_context* c) { c->meter_have = false; }

// The full-size guide of pt_upsample is forgotten (a new scene; a new camera, frame size or scale is seen by
// the call itself): the next pt_upsample renders it again.
inline void upsample_forget(pt_context* c) { c->up_scale = 0; }

// The adaptive state ends (a scene, light or params upload, a resize, a rebind, pt_clear_accum, any render):
// pt_adaptive_advance and the reads then ask for a new pt_adaptive_begin.  The buffers stay.
inline void adaptive_forget(pt_context* c) {
  c->ad_active = false;
  c->ad_var_valid = false;
}

// Before a launch that writes context-owned buffers: wait for the previous
// such launch if it ran on another stream.
inline int order_shared(pt_context* c) {
  if (c->shared_stream && c->shared_stream != c->stream) PT_HIP(hipStreamWaitEvent(c->stream, c->shared_ev, 0));
  return PT_OK;
}
// After enqueueing work that reads or writes context-owned buffers on
// c->stream: record it in that stream's use event (a context rarely sees more
// than a handful of streams; past kMaxUses the oldest entry is waited for and
// dropped).
constexpr size_t kMaxUses = 16;
inline int note_use(pt_context* c) {
  for (auto& u : c->uses)
    if (u.stream == c->stream) {
      PT_HIP(hipEventRecord(u.ev, c->stream));
      return PT_OK;
    }
  if (c->uses.size() >= kMaxUses) {
    PT_HIP(hipEventSynchronize(c->uses.front().ev));
    PT_HIP(hipEventDestroy(c->uses.front().ev));
    c->uses.erase(c->uses.begin());
  }
  pt_context::Use u{c->stream, nullptr};
  PT_HIP(hipEventCreateWithFlags(&u.ev, hipEventDisableTiming));
  c->uses.push_back(u);
  PT_HIP(hipEventRecord(u.ev, c->stream));
  return PT_OK;
}
// After it (or after the last launch that reads those buffers back).
inline int mark_shared(pt_context* c) {
  PT_HIP(hipEventRecord(c->shared_ev, c->stream));
  c->shared_stream = c->stream;
  return note_use(c);
}
// Before buffers that launches on any stream may still read are freed or
// overwritten from the host (list rebuilds, reallocation): wait for this
// context's own work on every stream it used -- not for the whole device.
inline int quiesce(pt_context* c) {
  for (auto& u : c->uses) PT_HIP(hipEventSynchronize(u.ev));
  return PT_OK;
}

// A library-owned device buffer of at least n elements; *cap counts the
// elements *p holds.  What it held is not kept.
template <class T>
int grow_dev(pt_context* c, T** p, size_t* cap, size_t n) {
  if (*p && *cap >= n) return PT_OK;
  { const int rc_ = quiesce(c); if (rc_) return rc_; }
  dev_free(*p);
  *cap = 0;
  PT_HIP(hipMalloc((void**)p, n * sizeof(T)));
  *cap = n;
  return PT_OK;
}

// A call wrote the image dst at the caller's request: if that is the
// accumulation buffer, what its culled items hold and the moments that went
// with it are no longer known.
inline void accum_overwritten(pt_context* c, const void* dst) {
  if (dst != (const void*)c->d_accum) return;
  c->culled_state = 0;
  c->moments_valid = false;
}

// Copies a library-owned W x H image of `per` floats a pixel to the host behind the work enqueued so far.
inline int read_image(pt_context* c, const void* img, int w, int h, int per, float* out, size_t n) {
  const size_t need = (size_t)w * h * per;
  if (n < need) return fail(PT_ERR_INVALID, "output buffer too small: need " + std::to_string(need) + " floats");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(hipMemcpyAsync(out, img, need * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  PT_HIP(hipStreamSynchronize(c->stream));
  return PT_OK;
}

// ---- what the core (pt_api.cpp) gives pt_post.cpp (a launch's scene, frame and camera fields, the
// camera block alone, and the wide-walk arrays) ...
void frame_params(const pt_context* c, bool full_nodes, ptd::RenderParams* p);
void camera_params(const float cam[16], ptd::RenderParams* p);
int wide_params(pt_context* c, ptd::RenderParams* p);
// ... and pt_dist.cpp: one frame of the step loop is render_impl with a packed output and an
// optional gathered frame to assemble, or a relaunch of an earlier such frame's parameters.
struct Assembly {   // pt_render_packed's optional gathered frame to assemble
  const void* src = nullptr;
  size_t slot_floats = 0;
  void* frame = nullptr;
};
// The parameters of a path-recursive launch as render_impl made it, so that
// pt_dist_run can launch the next frames of a run (same scene, camera,
// options and item layout; only the packed output and the frame to assemble
// change) without rebuilding them: the host cost of a frame is then the
// launch and its events (relaunch).
struct Launched {
  ptd::RenderParams p;
  bool lds = false, cnt = false, valid = false;
};
int render_impl(pt_context* c, uint32_t first_batch, uint32_t n_batches, float4* pack_out,
                const Assembly& as = Assembly(), Launched* launched = nullptr);
int relaunch(pt_context* c, const ptd::RenderParams& p, bool lds, bool cnt);
const ptd::Part& part_of(pt_context* c, int r);
void item_lists(const ptd::RenderParams& p, const ptd::Part& part, std::vector<int>* live,
                std::vector<int>* culled);
void frame_key(const pt_context* c, const ptd::RenderParams& p, std::vector<float>* key);
int unpack_table(pt_context* c, const ptd::RenderParams& p, const std::vector<float>& key);

// ---- and what they give the core --------------------------------------------------------------
void post_release(pt_context* c);      // frees what pt_post.cpp allocates (pt_destroy)
void adaptive_release(pt_context* c);  // ... and pt_adaptive.cpp
void display_release(pt_context* c);   // ... and pt_display.cpp
void rays_release(pt_context* c);      // ... and pt_rays.cpp
void upsample_release(pt_context* c);  // ... and pt_upsample.cpp
void radiance_release(pt_context* c);  // ... and pt_radiance.cpp
// ---- what the core gives pt_radiance.cpp: the wavefront pipeline's path buffers, grown to hold `paths` paths
// (they are the renders' own: a query between two renders finds them, or leaves them larger); b->cap = paths
int radiance_wf_buffers(pt_context* c, long long paths, ptd::WfBuffers* b);
// ---- what pt_post.cpp gives pt_upsample.cpp: the parameters of a guide launch of the context's scene and camera
// for a width x height frame as pt_render_guide makes them (the walk its rules choose, the wide walk's arrays
// grown); *lds: the scene is staged in LDS.  The checks of pt_render_guide are the caller's.
int guide_launch_params(pt_context* c, int width, int height, ptd::RenderParams* p, bool* lds);
// ... and pt_display.cpp: the metering launch of a w x h source (buffers grown, the state advanced); the state the
// display kernels read
int display_meter(pt_context* c, const pt_display_params& p, const float4* src, int w, int h);
int display_checked_params(const pt_display_params* in, pt_display_params* p);
// ---- what pt_post.cpp gives pt_adaptive.cpp: the variance-guided filter's passes from a variance plane
// (pt_post.cpp var_filter), and the validated filter parameters
int post_var_filter(pt_context* c, const pt_denoise_var_params& p, const float4* src, const float* var0,
                    const float4* guide, float4* dst);
int post_denoise_var_params(const pt_denoise_var_params* in, pt_denoise_var_params* p);
// ---- what the core gives pt_adaptive.cpp: the checks and the parameters of a path-recursive launch of the
// whole frame under an adaptive plan (no item list, no fill; the cull rectangles as render_impl derives them)
struct AdaptivePlan;
int adaptive_render_params(pt_context* c, const AdaptivePlan& ap, int spl, ptd::RenderParams* p);
// ... and a round on the wavefront pipeline (ap.wf): batches p->first_batch .. + p->n_batches of the live list,
// in path buffers reserved for every tile's pixels and reserve_batches batches (the same in every round of a
// render, so the rounds do not reallocate)
int adaptive_launch_wavefront(pt_context* c, const AdaptivePlan& ap, uint32_t reserve_batches, ptd::RenderParams* p);
int dist_synchronize(pt_context* c);   // pt_synchronize's share of the step loop: its render and gather streams

#pragma GCC visibility pop
