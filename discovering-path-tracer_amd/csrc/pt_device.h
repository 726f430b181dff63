// Device-side data layout and kernel launchers (host-visible declarations).
//
// HBM layout (all 16-B aligned, built once per scene upload):
//   nodes : 2 x float4 per BVH node, renumbered in the reference traversal's
//           visiting order (right child first, raytrace_comp.comp:198-199):
//             [0] = {min.x, min.y, min.z, skip}     skip = int bits
//             [1] = {max.x, max.y, max.z, tri}      tri  = int bits, -1 internal
//           An internal node whose box is hit continues at k+1 (its right
//           child); a missed node or a leaf continues at `skip`, the node the
//           reference's stack would pop next.  Same visit sequence, no stack.
//   tris  : 3 x float4 per triangle slot (slot = the reference's triIdx, the
//           row of the BVH-reordered index buffer):
//             {v0.xyz, e1.x} {e1.yz, e2.xy} {e2.z, n.xyz}
//           e1 = v1-v0, e2 = v2-v0 and n = normalize(cross(e1,e2)) are exactly
//           the values the reference recomputes per test (:119-120, :189).
//   accum : float4[H][W], RGBA32F running mean.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptd {

struct LightRec {          // == pt_area_light / AreaLightData
  float position[4];
  float normal[4];
  float intensity[4];
  float size[4];
};

// Light with its sampling frame precomputed on the device (setup_lights_kernel).
struct LightDev {
  float pos[3], nraw[3], inten[3], right[3], up[3], size[2], half[2];
  float finite;   // 1 when every intensity channel is finite (shadow_needed)
};

// Partition order of the 16x16 blocks: tile b is block row by = b / blocks_x,
// column (b % blocks_x + by) % blocks_x -- each row rotated by its index, so
// "b % nranks == rank" deals every rank anti-diagonal stripes of the image.
// (Row-major order gives column stripes whenever blocks_x % nranks == 0, and
// a centred object then lands unevenly: box.obj 1080p at 8 ranks put 5.7 %
// more of the geometry on rank 0 than the mean; rotated, 0.1 %.)
__host__ __device__ inline void tile_block(int b, int blocks_x, int* bx, int* by) {
  *by = b / blocks_x;
  *bx = (b % blocks_x + *by % blocks_x) % blocks_x;
}
__host__ __device__ inline int block_tile(int bx, int by, int blocks_x) {
  return by * blocks_x + (bx - by % blocks_x + blocks_x) % blocks_x;
}

// A rank's tiles under a slotted partition: tiles are dealt in periods of m
// slots and a rank owns cnt of them, at the ascending positions pos[] of each
// period, i.e. tile b iff b % m is one of pos[].  One slot per rank (m =
// nranks, pos = {rank}) is "b % nranks == rank".  Unequal slot counts let the
// root, which also assembles the frame, render a smaller share
// (pt_set_partition_slots); the host spreads every rank's slots evenly over
// the period, since runs of neighbouring tiles would land unevenly on a
// centred object.
constexpr int kMaxSlots = 64;
struct Part {
  int m, cnt;
  int pos[kMaxSlots];
};
__host__ __device__ inline int part_tile(const Part& p, int li) { return (li / p.cnt) * p.m + p.pos[li % p.cnt]; }
__host__ __device__ inline int part_count(const Part& p, int total) {
  const int rem = total % p.m;
  int n = (total / p.m) * p.cnt;
  for (int i = 0; i < p.cnt; ++i) n += p.pos[i] < rem ? 1 : 0;
  return n;
}
__host__ __device__ inline bool part_owns(const Part& p, int b) {
  const int v = b % p.m;
  bool own = false;
  for (int i = 0; i < p.cnt; ++i) own = own || p.pos[i] == v;
  return own;
}

struct RenderParams {
  // culled wide walk (wide_walk.h), or null: 4-wide nodes, triangle records
  // by leaf rank, triangle slot -> rank, per-lane stack overflow areas
  // (wide_ovf_lanes lanes of wide_stack entries, lane-strided)
  const float4* hit_tris;   // the records a closest hit's index refers to: wide_tris (by rank) with the wide walk, else tris
  const float4* wide;        // 64-B nodes when wide_qn 1, else 128-B (wide_walk.h)
  int wide_qn;
  const float4* wide_leafbox;   // wide_qn: the reference's leaf box per rank, 2 float4
  const float4* wide_tris;
  const int* wide_rank_of;
  int2* wide_ovf;
  long long wide_ovf_lanes;
  int wide_stack;
  int wide_handback;        // test: hand every odd list slot to the exact walk (PT_OPT_WIDE 2)
  int wf_fuse;              // PT_OPT_WF_FUSE: the wide trace kernel also walks a closest hit's first-light shadow ray
  int wf_tail;              // PT_OPT_WF_TAIL: a list of fewer rays than this is finished by wf_tail_kernel (0: never)
  int wf_grid;              // PT_OPT_WF_GRID: the persistent traversal grid in percent of a full-occupancy grid (1-100)
  int wide_refill;          // PT_OPT_WF_REFILL: idle lanes at which a wave of the wide trace kernel refills
  const float4* nodes;
  const float4* tris;
  // the sweep table of a tiny scene (sweep_walk.h SweepTable, PT_OPT_SMALL_SWEEP)
  // or null: render_kernel<false, true, false, 1 or 2> then walks it instead of nodes
  const float4* sweep = nullptr;
  int sweep_boxes = 0, sweep_leaves = 0;
  int sweep_hull = 0;   // host only: the table holds hull codes (PT_OPT_SWEEP_HULL), which picks the kernel that reads them
  const LightDev* lights;
  float4* accum;
  // [0..3] rays, nodes, leaf tests, samples (stats mode); [4..8] closest walks,
  // shadow walks, nodes visited, triangle tests, primaries (counting mode)
  unsigned long long* stats;
  int n_nodes;
  int n_tris;
  int n_lights;
  int width, height;
  uint32_t first_batch, n_batches;
  int max_depth, sss_bounces;
  float cam_pos[3], cam_dir[3], cam_up[3], fov;
  // camera frame of main() (:430-432) computed on the host with pt_math.h:
  // right = normalize(cross(dir, -up)), up' = normalize(cross(right, dir)),
  // tan(radians(fov * 0.5))
  float cam_right[3], cam_upv[3], tan_fov;
  int blocks_x, blocks_total;   // 16x16-pixel blocks
  int nranks, rank;             // this rank of nranks
  // its tiles (Part on the host): the period, its slot count, its slot
  // positions in device memory (rank_tile), and how many tiles it owns
  int part_m, part_cnt, n_tiles;
  const int* part_pos;
  int spl;                      // sample lanes per pixel: 1, 2, 4 or 8
  int fresh;                    // first_batch == 0 starts from +0 without reading accum
  // primary-ray culling (pt_primary_cull_rects): -1 = trace every pixel; else
  // a pixel traces only if its NDC origin lies in one of cull[0..n_cull)
  // compact launch (host-built when culling applies): items (owned tile *
  // spl + part) that may hold a live pixel, and those that cannot
  const int* items;             // null = every item, blockIdx.x = item
  const int2* items_org;        // with items: per live item its first pixel {x, y} (host-computed)
  int n_items;
  const int2* culled_org;       // per culled item: its first pixel {x, y} (host-computed)
  int n_culled_items;
  int n_cull;
  float cull[8][4];
  // the tight rectangles (pt_cull.h, PT_OPT_CULL_TIGHT): derived like cull[] but for radii of at most
  // kCullTightR; -1 = none.  Outside all of them a sample whose two radius draws u1 are at least cull_u0
  // (kCullTightU0: both radii within the bound) is (0,0,0) and is not traced.  Kernel only: the host's
  // item lists, fills and partitions go by cull[]
  int n_cull_tight = -1;
  float cull_tight[8][4] = {};
  float cull_u0 = 0.0f;
  // pt_render_packed: live workgroup i stores its pixels to pack_out[i*256/spl
  // + q] (the pt_items_pack layout) instead of the accumulation buffer, and no
  // culled-item fill runs; null = normal rendering
  float4* pack_out;
  // ... and, optionally, trailing workgroups that assemble a gathered frame
  // (the pt_items_unpack_all work: int4 table entries {rank, x0, y0, slot}
  // -- the item's first pixel, its slot or -1 for a culled item -- over
  // per-rank slots of unpack_slot_f4 float4s) in the same launch
  const float4* unpack_src;
  float4* unpack_frame;
  const int* unpack_table;
  int n_unpack;
  long long unpack_slot_f4;
  int item_order;   // host only: PT_OPT_ITEM_ORDER for the item lists
  // mixed sample lanes (PT_OPT_MIXED_LANES, one-rank path-recursive launches
  // with items): live item i is items_org[i] = {x | log2(spl_i) << 24, y}, a
  // whole 16x16 tile at one lane per pixel or a part at `spl` lanes; the
  // culled items keep `spl`
  int mix = 0;
  // per 16x4 part of the frame (y / 4 * blocks_x + x / 16): the summed wave
  // durations of the launch's live workgroups in GPU wall-clock ticks, or null
  unsigned* cost_out = nullptr;
  // luminance moments (PT_OPT_MOMENTS): float2 {m1, m2} per pixel of the frame, folded beside the colour
  // by the MOMENTS instantiations (launch_render / launch_wavefront pick them when this is set); the live
  // pixels only -- the host zeroes the image before a launch from batch 0, and a culled pixel's fold of
  // L = +0 into +0 is +0.  After every older member: the layout the other instantiations read does not move
  float2* moments = nullptr;
  // the exit skip (PT_OPT_EXIT_SKIP, pt_isect.h exit_skip): set by the host when the option is on, some
  // triangle's stored normal is axis-pure (exit_normal) and every light is finite; the fast path tracers
  // then end a path whose bounce ray provably leaves through a face of the root box [root_lo, root_hi]
  // (node 0 of the reference's tree, bitwise).  Clear: no kernel evaluates the predicate -- the LDS-staged
  // render kernels branch on it, the others are the instantiations without it (launch_render,
  // launch_wavefront), which read nothing past `moments`
  int exit_skip = 0;
  float root_lo[3] = {}, root_hi[3] = {};
  // the seed base (PT_OPT_SEED_BASE): sample s of the launch draws from the seed ((first_batch + seed_base
  // + s) * H + py) * W + px in uint32 arithmetic and still folds with weight first_batch + s.  0: the seeds
  // of before.  Read at the seed sites only (render_kernel, the generation kernel's tight-cull draw,
  // path_step's PH_BEGIN), as one scalar add to first_batch: of the ways tried (the product B * H * W added
  // to the seed; first_batch + B formed on the host) the one that moved the kernels' code least
  // (profiles/temporal/resource_usage.md).  It sits in the struct's tail padding: the kernel argument
  // keeps its size
  uint32_t seed_base = 0;
  // the cube table (PT_OPT_SWEEP_CUBE, sweep_walk.h sweep_cands_cube): the under words of the root box's six
  // faces in the order x lo, x hi, y lo, y hi, z lo, z hi (0: the table has no such face) and the root's own;
  // the root box itself is root_lo / root_hi above.  Read by the SWEEP 3 instantiations only, as one run of words
  // from root_lo to cube_all (kernels/walks.h sweep_cube_words: keep them adjacent); after every older member.
  // sweep_cube: host only, picks those instantiations (launch_render)
  uint32_t cube_under[6] = {};
  uint32_t cube_all = 0;
  int sweep_cube = 0;
  // the footprint table (pt_cull.h, PT_OPT_CULL_FOOTPRINT), read by pixel_skip only; after every older member.
  // foot: device memory, kMaxCullRects footprints and then kMaxCullRects sure regions of kFootprintFloats
  // floats each (a rectangle and kFootprintPlanes half-planes).
  // n_foot > 0: a pixel outside every one of footprints 0 .. n_foot - 1 skips its samples with both radius
  // draws at least cull_u0 as black, in place of a pixel outside every tight rectangle; 0: the rectangles decide.
  // n_sure > 0: lights 0 .. n_sure - 1 have a sure region (maybe an empty one); a pixel in light l's region and
  // in no footprint but that light's own (footprint l + 1) skips those samples as (intensity, 1), in
  // render_kernel and the wavefront generation kernel.
  // A table like `sweep`, not words of the argument: the LDS kernels keep the whole argument in scalar
  // registers, and 97 more words cost them 90 spilled SGPRs and, with the option off, 2 % of their time
  // (profiles/footprint/resource_usage.md).
  int n_foot = 0;
  int n_sure = 0;
  const float* foot = nullptr;
};
constexpr int kMixShift = 24;
constexpr int kMaxCullRects = 8;
constexpr int kStatsWords = 9;   // RenderParams::stats

hipError_t launch_setup_tris(const float* d_vertices, const uint32_t* d_indices, int n_tris, float4* d_tris,
                             hipStream_t stream);
hipError_t launch_setup_lights(const LightRec* d_in, int n, LightDev* d_out, hipStream_t stream);
int owned_tiles(int width, int height, const Part& part);
hipError_t launch_tiles(bool pack, float4* frame, float4* packed, int width, int height, const Part& part,
                        const int* d_pos,
                        hipStream_t stream);
hipError_t launch_clear(float4* accum, int width, int height, const Part& part, const int* d_pos, hipStream_t stream);
// live-item exchange: pack this rank's listed items (256/spl pixels each) of
// frame densely; unpack int4 entries {rank, x0, y0, slot} from per-rank slots
// of slot_f4 float4s into frame, slot -1 = culled item -> (0,0,0,1)
hipError_t launch_items_pack(const RenderParams& p, const float4* frame, float4* packed, const int* items, int n,
                             hipStream_t stream);
hipError_t launch_items_unpack(const RenderParams& p, float4* frame, const float4* src, size_t slot_f4,
                               const int* table, int n, hipStream_t stream);
// Scene bytes the LDS-staged variant needs, and the largest it accepts.
constexpr size_t kMaxSceneLds = 48 * 1024;
inline size_t scene_lds_bytes(const RenderParams& p) {
  return ((size_t)2 * p.n_nodes + (size_t)3 * p.n_tris) * 16;
}
// ... and what the sweep walk stages: the triangle records, by leaf
inline size_t sweep_lds_bytes(const RenderParams& p) { return (size_t)3 * p.sweep_leaves * 16; }
// cnt: the fast kernel with traced-work counters (PT_OPT_COUNT_TRACED)
hipError_t launch_render(const RenderParams& p, bool stats, bool lds_scene, hipStream_t stream, bool cnt = false);
// One adaptive round (kernels/adaptive.h): blocks_total * spl workgroups; workgroup i serves part i % spl of
// list[i / spl] = {x0, y0, first_batch, n_batches} and leaves when i / spl >= *n_live (both device memory).
hipError_t launch_render_adaptive(const RenderParams& p, bool lds_scene, const int4* list, const int* n_live,
                                  hipStream_t stream);
// Wavefront pipeline (PT_OPT_KERNEL 3): one path per (pixel, sample) held in
// HBM; generate, then alternate a persistent traversal kernel over the list of
// paths waiting for a ray and a shading kernel that consumes the hits and
// emits the next rays; finally fold each pixel's sample colours in batch
// order.  Buffers hold `cap` paths; larger launches run in batch chunks.
struct WfBuffers {
  float4* state[2];  // per list slot: the fields of the waiting path's PathSt its phase needs, by component
                     // (chunk j of slot s at [j * cap + s], wf_store_state)
  float4* colors;    // per path radiance
  int* ids[2];       // work lists: path id per slot
  float4* rays[2];   // ... and its ray, 2 float4 per slot: {o.xyz, limit} {d.xyz, shadow}
  float2* hits;      // per slot of the list being traced: {t, tri bits / occluded}
  int* counters;     // [0],[1] list sizes, [2] trace fetch cursor ([4..6]: the second half's, two streams)
  long long cap;     // paths the buffers hold
};
constexpr int kWfStateF4 = 9;   // state chunks (float4) a waiting path stores at most
// kind word of a listed ray (rays[cap + s].w): 0 closest, 1 shadow, 2 null
// shadow query, plus (PT_OPT_WF_FUSE, closest rays) kRayFuse: the trace
// kernel walks the path's first-light shadow ray after a hit (the ray's
// limit word then holds the path's RNG state); kRayPrimary: a primary ray,
// whose light pre-pass (raytrace_comp.comp:311-328) may end the path first
constexpr int kRayKindMask = 3, kRayFuse = 4, kRayPrimary = 8;
// hits[s].y of a fused closest hit: rank | kHitFused | (kHitOccluded if the
// shadow ray was occluded)
constexpr int kHitFused = 0x40000000, kHitOccluded = 0x20000000, kHitRankMask = 0x1fffffff;
constexpr size_t kWfBytesPerPath = 2 * (size_t)kWfStateF4 * 16 + 16 + 2 * (4 + 32) + 8;
// rays a path may trace in one sample: the primary ray, then per bounce the
// light shadow rays, sss_bounces x (walk ray + light shadow rays) and the
// next bounce ray
inline int wf_max_rays(const RenderParams& p) {
  return 1 + p.max_depth * (p.n_lights + p.sss_bounces * (1 + p.n_lights) + 1);
}
// stream2 (with two events): the chunk's pixels run as two halves on stream
// and stream2 (forked from and joined back into stream); the wide walk's
// overflow area then holds two sets of wide_ovf_lanes lanes.
hipError_t launch_wavefront(const RenderParams& p, const WfBuffers& b, bool lds_scene, hipStream_t stream,
                            bool cnt = false, hipStream_t stream2 = nullptr, hipEvent_t ev_fork = nullptr,
                            hipEvent_t ev_join = nullptr);
// One adaptive round on the wavefront pipeline (PT_OPT_ADAPTIVE_WF, kernels/wf_adaptive.h): batches
// p.first_batch .. + p.n_batches of the tiles list[0 .. *n_live) (both device memory), on one stream.
hipError_t launch_wavefront_adaptive(const RenderParams& p, const WfBuffers& b, bool lds_scene, const int4* list,
                                     const int* n_live, hipStream_t stream);
// First-hit guide image of the whole frame (pt_render_guide): float4 {n.xyz, t}
// per pixel from p's camera, size and scene.  p.wide set: the culled wide
// walk; else the exact walk, staged in LDS with lds_scene.
hipError_t launch_guide(const RenderParams& p, float4* guide, bool lds_scene, hipStream_t stream);
// Batched ray queries (pt_trace_rays, kernels/rays.h): n rays of 2 float4 {o.xyz, d.x} {d.yz, limit, -} into n
// closest hits of 2 float4 {t, tri, u, v} {n.xyz, 0} (kRaysClosest) or n occlusion words (kRaysAny), from p's
// scene alone.  p.wide set: the culled wide walk in the shape `refill` picks (PT_OPT_RAYS_REFILL), then the
// exact walk over the rays it marked; else the exact walk, staged in LDS with lds_scene.  counters: two
// library-owned words (the ray cursor, the marks), cleared here on the stream; slot_of: rank -> triangle index
// of p's wide tree (launch_rays_slots), read with p.wide only.
constexpr int kRaysClosest = 0, kRaysAny = 1;   // == PT_RAYS_CLOSEST, PT_RAYS_ANY
hipError_t launch_rays(const RenderParams& p, int kind, const void* rays, size_t n, void* out, uint32_t* counters,
                       const int* slot_of, bool lds_scene, bool refill, hipStream_t stream);
hipError_t launch_rays_slots(const int* rank_of, int n, int* slot_of, hipStream_t stream);
// Radiance queries (pt_trace_radiance, kernels/radiance.h): one chunk, queries q0 .. q0 + n_queries of `rays`
// (2 float4 each: {o.xyz, d.x} {d.yz, -, seed}), n_samples samples each from the seeds seed + s * seed_stride,
// folded into out[q0 ..] (one float4 a query).  p: the scene, lights, parameters and walk choices (plan_radiance).
// launch_radiance: the path-recursive kernel; colors holds n_queries * n_samples float4, library-owned.
// launch_wavefront_rays: the wavefront pipeline's rounds behind wf_gen_rays_kernel, in b (cap >= the paths).
hipError_t launch_radiance(const RenderParams& p, bool lds_scene, const void* rays, long long q0, long long n_queries,
                           uint32_t n_samples, uint32_t seed_stride, float4* colors, void* out, hipStream_t stream);
hipError_t launch_wavefront_rays(const RenderParams& p, const WfBuffers& b, bool lds_scene, const void* rays,
                                 long long q0, long long n_queries, uint32_t n_samples, uint32_t seed_stride, void* out,
                                 hipStream_t stream);
// main()'s own rays of p's camera and size as queries (pt_camera_rays): n entries of pixels (null: every pixel
// in raster order) for sample batch `batch`.
hipError_t launch_camera_rays(const RenderParams& p, uint32_t batch, const int* pixels, long long n, void* rays,
                              hipStream_t stream);
// One pass of the a-trous filter (pt_denoise.h atrous_pixel) from src to dst
// (distinct images) at tap spacing `step` with the pass's squared sigmas;
// staged: the tile and its halo go through LDS (steps 1 and 2 only).
hipError_t launch_atrous(const float4* src, const float4* guide, float4* dst, int width, int height, int step,
                         float sc2, float sn2, float sz2, bool staged, hipStream_t stream);
// The variance-guided filter (pt_denoise.h atrous_var_pixel): var0 from the
// moments of n_samples >= 2 samples, then one pass from (src, vsrc) to (dst,
// vdst), all four distinct; staged as above.
hipError_t launch_moments_var(const float2* moments, float* var, int width, int height, uint32_t n_samples,
                              hipStream_t stream);
hipError_t launch_atrous_var(const float4* src, const float* vsrc, const float4* guide, float4* dst, float* vdst,
                             int width, int height, int step, float sigma_lum, float sn2, float sz2, bool staged,
                             hipStream_t stream);
// Temporal reprojection (pt_denoise.h reproject_pixel): the frame of n samples (color, moments, guide from
// cam_cur) blended with the history images (from cam_prev; all four null: no history) into the four output
// images, distinct from every input.
hipError_t launch_reproject(const float4* color, const float2* moments, const float4* guide, const float4* hist_color,
                            const float2* hist_moments, const float* hist_length, const float4* hist_guide,
                            float4* out_color, float2* out_moments, float* out_length, float* out_variance,
                            const float cam_cur[16], const float cam_prev[16], int width, int height, uint32_t n,
                            uint32_t max_history, float alpha_min, float normal_min, float depth_rel,
                            hipStream_t stream);
// lanes of the wide walk's persistent grid on this device (overflow areas to allocate)
long long wide_trace_lanes();
// workgroups of the LDS-staged render kernel resident on this device at once
long long render_slots(size_t lds_bytes, bool sweep = false);   // sweep: of its sweep-walk variant
// triangle records by rank: dst[r] = tris[tri_of[r]]
hipError_t launch_gather_tris(const float4* tris, const int* tri_of, int n, float4* dst, hipStream_t stream);
hipError_t launch_math(int fn, const float* x, float* y, size_t n, hipStream_t stream);
hipError_t launch_exhaustive(int fn, unsigned long long* bad, uint32_t* first_bad, hipStream_t stream);

// ---------------------------------------------------------------------------
// Kernel selection.  What launch_render and launch_wavefront refuse, the grid
// and dynamic LDS they launch with and the instantiation they run are pure
// functions of the parameters: they call no HIP function and launch nothing,
// so a host program table-tests them (tests/plan_check.cpp, tests/test_plan.py)
// -- most instantiations give bit-identical frames, and no GPU test would
// notice the wrong one.  Each kernel family's instantiations are listed once,
// here; pt_device.hip builds its table of kernels from the same list, and a
// variant that is not listed is hipErrorInvalidValue.
// ---------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
struct RenderVariant {     // render_kernel<STATS, LDS, CNT, SWEEP, MOMENTS, EXIT>
  bool stats, lds, cnt;
  int sweep;
  bool moments, exit;
};
struct WfTraceVariant {    // wf_trace_kernel<LDS, G, CNT>
  bool lds;
  int group;
  bool cnt;
};
struct WfWideVariant { bool qn, cnt; };          // wf_trace_wide_kernel<CNT, LAYOUT = qn>
struct WfShadeVariant { bool exit; };            // wf_shade_kernel<EXIT>
struct WfTailVariant { bool cnt, qn, exit; };    // wf_tail_kernel<CNT, QN, EXIT>
constexpr bool operator==(const RenderVariant& a, const RenderVariant& b) {
  return a.stats == b.stats && a.lds == b.lds && a.cnt == b.cnt && a.sweep == b.sweep && a.moments == b.moments &&
         a.exit == b.exit;
}
constexpr bool operator==(const WfTraceVariant& a, const WfTraceVariant& b) {
  return a.lds == b.lds && a.group == b.group && a.cnt == b.cnt;
}
constexpr bool operator==(const WfWideVariant& a, const WfWideVariant& b) { return a.qn == b.qn && a.cnt == b.cnt; }
constexpr bool operator==(const WfShadeVariant& a, const WfShadeVariant& b) { return a.exit == b.exit; }
constexpr bool operator==(const WfTailVariant& a, const WfTailVariant& b) {
  return a.cnt == b.cnt && a.qn == b.qn && a.exit == b.exit;
}

// The instantiations that exist, X(template arguments in the struct's order).  The kernels lie in the code
// object in the order they are listed in: keep it when the object is to be compared with an earlier one.
#define PT_RENDER_VARIANTS(X)                                                                                  \
  X(false, true, false, 2, true, false) X(false, true, false, 1, true, false)     /* moments: the sweep walks, */ \
  X(false, true, false, 3, true, false) X(false, false, false, 0, true, true)     /* device memory, LDS */        \
  X(false, false, false, 0, true, false) X(false, true, false, 0, true, false)                                    \
  X(false, true, false, 2, false, false) X(false, true, false, 1, false, false)   /* the sweep walks */           \
  X(false, true, false, 3, false, false)                                                                          \
  X(false, false, true, 0, false, true) X(false, false, true, 0, false, false)    /* counting */                  \
  X(false, true, true, 0, false, false)                                                                           \
  X(true, true, false, 0, false, false) X(false, true, false, 0, false, false)    /* stats and plain */           \
  X(false, false, false, 0, false, true) X(false, false, false, 0, false, false)                                  \
  X(true, false, false, 0, false, false)
#define PT_WF_WIDE_VARIANTS(X) X(true, false) X(true, true) X(false, false) X(false, true)
#define PT_WF_TRACE_VARIANTS(X)                                                                \
  X(true, 2, true) X(true, 4, true) X(false, 2, true) X(false, 4, true) X(true, 2, false)      \
  X(true, 4, false) X(false, 2, false) X(false, 4, false)
#define PT_WF_SHADE_VARIANTS(X) X(true) X(false)
#define PT_WF_TAIL_VARIANTS(X)                                                              \
  X(true, true, true) X(false, true, true) X(true, false, true) X(false, false, true)       \
  X(true, true, false) X(false, true, false) X(true, false, false) X(false, false, false)
#define PT_VARIANT_ROW(...) {__VA_ARGS__},
constexpr RenderVariant kRenderVariants[] = {PT_RENDER_VARIANTS(PT_VARIANT_ROW)};
constexpr WfTraceVariant kWfTraceVariants[] = {PT_WF_TRACE_VARIANTS(PT_VARIANT_ROW)};
constexpr WfWideVariant kWfWideVariants[] = {PT_WF_WIDE_VARIANTS(PT_VARIANT_ROW)};
constexpr WfShadeVariant kWfShadeVariants[] = {PT_WF_SHADE_VARIANTS(PT_VARIANT_ROW)};
constexpr WfTailVariant kWfTailVariants[] = {PT_WF_TAIL_VARIANTS(PT_VARIANT_ROW)};
#undef PT_VARIANT_ROW
template <class V, size_t N>
constexpr int variant_index(const V (&list)[N], const V& v) {   // -1: no such instantiation
  for (size_t i = 0; i < N; ++i)
    if (list[i] == v) return (int)i;
  return -1;
}

// The flags' share of launch_render's decision.  sweep_table: 0 no sweep table, 1 a general one, 2 one with
// hull faces, 3 the cube table; the sweep walk is the plain LDS kernel's only.  exit_skip: device-memory
// scenes take the EXIT instantiations, the LDS-staged kernels branch on P.exit_skip instead.
struct RenderPick {
  bool ok;   // false: refused
  RenderVariant v;
};
constexpr RenderPick pick_render(bool stats, bool lds_scene, bool cnt, int sweep_table, bool moments, bool exit_skip,
                                 bool pack_out) {
  if ((cnt && stats) || (pack_out && stats) || (moments && (stats || cnt || pack_out))) return {false, {}};
  const int sweep = lds_scene && !stats && !cnt ? sweep_table : 0;
  return {true, {stats, lds_scene, cnt, sweep, moments, exit_skip && !stats && !lds_scene}};
}

constexpr bool spl_valid(int spl) { return spl == 1 || spl == 2 || spl == 4 || spl == 8; }
enum class Launch { Refused, Nothing, Run };   // Refused: hipErrorInvalidValue; Nothing: success, no work
struct RenderLaunch {
  Launch what = Launch::Refused;
  long long grid = 0;   // workgroups (0 with Run: a compact launch that lists no item; nothing is launched)
  size_t lds = 0;       // dynamic LDS bytes
  RenderVariant v = {};
};
// pix_per_fill: the render kernel's kPixPerFill (pixels per thread of its trailing workgroups).
inline RenderLaunch plan_render(const RenderParams& p, bool stats, bool lds_scene, bool cnt, int pix_per_fill) {
  RenderLaunch l;
  if ((cnt && stats) || !spl_valid(p.spl)) return l;
  // owned tiles (part_tile); the recursive kernel splits each into spl workgroups
  l.grid = (long long)p.n_tiles * p.spl;
  if (l.grid <= 0 || p.n_batches == 0) {
    l.what = Launch::Nothing;
    return l;
  }
  // live items (p.n_items), then the trailing workgroups: with pack_out those that assemble the previous
  // frame, with a compact list (p.items) those that fill the culled items
  const long long trailing_px = (long long)(p.pack_out ? p.n_unpack : p.n_culled_items) * (256 / p.spl);
  if (p.pack_out || p.items) l.grid = p.n_items + (trailing_px + 256 * pix_per_fill - 1) / (256 * pix_per_fill);
  if (l.grid > 0x7fffffffll) return l;
  const int table = !p.sweep ? 0 : p.sweep_cube ? 3 : p.sweep_hull ? 2 : 1;
  const RenderPick pick = pick_render(stats, lds_scene, cnt, table, p.moments != nullptr, p.exit_skip != 0,
                                      p.pack_out != nullptr);
  if (!pick.ok) return l;
  if (pick.v.sweep && (p.sweep_boxes < 1 || p.sweep_boxes > 64 || p.sweep_leaves < 1 || p.sweep_leaves > 32)) return l;
  l.lds = pick.v.sweep ? sweep_lds_bytes(p) : lds_scene ? scene_lds_bytes(p) : 0;
  if (l.lds > kMaxSceneLds) return l;
  l.v = pick.v;
  l.what = Launch::Run;
  return l;
}

// ... and of launch_wavefront's.  wide: the culled wide walk is set up (p.wide); it traces device-memory
// scenes only.  tail_wanted: p.wf_tail > 0 (wf_tail_kernel takes the short lists: the wide walk's layouts
// only -- the trace and shading kernels would skip its lists).  group2: fewer than kWfGroup4Tris triangles.
struct WfPick {
  bool ok, wide, tail;
  WfTraceVariant trace;   // !wide
  WfWideVariant wide_trace;   // wide
  WfShadeVariant shade;
  WfTailVariant tail_v;   // tail
};
constexpr WfPick pick_wavefront(bool lds_scene, bool wide, bool wide_qn, bool cnt, bool exit_skip, bool moments,
                                bool tail_wanted, bool group2) {
  const bool w = wide && !lds_scene;
  if ((moments && cnt) || (tail_wanted && !w)) return {false, false, false, {}, {}, {}, {}};
  return {true, w, w && tail_wanted, {lds_scene, group2 ? 2 : 4, cnt}, {wide_qn, cnt}, {exit_skip},
          {cnt, wide_qn, exit_skip}};
}
// Where launch_wavefront stops.  The culled items' fill is launched before the checks that need a live item,
// so a launch they refuse has run it (FillRefused), as has one without a live item (FillOnly).
enum class WfStop { Refused, Nothing, FillOnly, FillRefused, Run };
struct WfLaunch {
  WfStop stop = WfStop::Refused;
  long long fill_grid = 0;   // fill_culled_kernel's workgroups (0: not launched)
  long long px = 0;          // pixels of the live items
  size_t lds_trace = 0;      // the trace kernel's dynamic LDS bytes
  WfPick k = {};
};
// cap: WfBuffers::cap.  pix_per_fill as above; group4_tris: the trace kernel's kWfGroup4Tris.
inline WfLaunch plan_wavefront(const RenderParams& p, long long cap, bool lds_scene, bool cnt, int pix_per_fill,
                               int group4_tris) {
  WfLaunch l;
  if ((p.moments && cnt) || !spl_valid(p.spl)) return l;
  if (p.n_batches == 0) {
    l.stop = WfStop::Nothing;
    return l;
  }
  const int per = 256 / p.spl;
  const long long items = p.items ? p.n_items : (long long)p.n_tiles * p.spl;
  if (p.items && p.n_culled_items > 0)
    l.fill_grid = ((long long)p.n_culled_items * per + 256 * pix_per_fill - 1) / (256 * pix_per_fill);
  if (items <= 0) {
    l.stop = WfStop::FillOnly;
    return l;
  }
  l.stop = WfStop::FillRefused;
  l.px = items * per;
  if (l.px > cap || cap > 0x7fffffffll) return l;
  const size_t lds = lds_scene ? scene_lds_bytes(p) : 0;
  if (lds > kMaxSceneLds) return l;
  const WfPick k = pick_wavefront(lds_scene, p.wide != nullptr, p.wide_qn != 0, cnt, p.exit_skip != 0,
                                  p.moments != nullptr, p.wf_tail > 0, p.n_tris < group4_tris);
  if (!k.ok) return l;
  if (k.wide && p.wide_ovf_lanes < 256) return l;   // every lane needs its overflow stack area
  l.lds_trace = k.wide ? 0 : lds;
  l.k = k;
  l.stop = WfStop::Run;
  return l;
}

// ... and of launch_render_adaptive's (an adaptive round, kernels/adaptive.h): the MOMENTS instantiations
// of render_kernel have one sibling each, picked by the same rule (pick_render with moments and neither
// stats, counters nor a packed output).
struct AdaptiveVariant {   // render_adaptive_kernel<LDS, SWEEP, EXIT>
  bool lds;
  int sweep;
  bool exit;
};
constexpr bool operator==(const AdaptiveVariant& a, const AdaptiveVariant& b) {
  return a.lds == b.lds && a.sweep == b.sweep && a.exit == b.exit;
}
#define PT_ADAPTIVE_VARIANTS(X) \
  X(true, 2, false) X(true, 1, false) X(true, 3, false) X(false, 0, true) X(false, 0, false) X(true, 0, false)
#define PT_VARIANT_ROW(...) {__VA_ARGS__},
constexpr AdaptiveVariant kAdaptiveVariants[] = {PT_ADAPTIVE_VARIANTS(PT_VARIANT_ROW)};
#undef PT_VARIANT_ROW
constexpr AdaptiveVariant pick_adaptive(bool lds_scene, int sweep_table, bool exit_skip) {
  const RenderVariant v = pick_render(false, lds_scene, false, sweep_table, true, exit_skip, false).v;
  return {v.lds, v.sweep, v.exit};
}
struct AdaptiveLaunch {
  Launch what = Launch::Refused;
  long long grid = 0;   // workgroups: every tile's parts, whatever the live list holds
  size_t lds = 0;       // dynamic LDS bytes
  AdaptiveVariant v = {};
};
// The launch over the frame's blocks_total tiles at p.spl lanes; the batches are the list's, p's are not read.
inline AdaptiveLaunch plan_render_adaptive(const RenderParams& p, bool lds_scene) {
  AdaptiveLaunch l;
  if (!spl_valid(p.spl) || !p.moments || p.pack_out || p.items || p.mix || p.nranks != 1) return l;
  l.grid = (long long)p.blocks_total * p.spl;
  if (l.grid <= 0) {
    l.what = Launch::Nothing;
    return l;
  }
  if (l.grid > 0x7fffffffll) return l;
  const int table = !p.sweep ? 0 : p.sweep_cube ? 3 : p.sweep_hull ? 2 : 1;
  const AdaptiveVariant v = pick_adaptive(lds_scene, table, p.exit_skip != 0);
  if (v.sweep && (p.sweep_boxes < 1 || p.sweep_boxes > 64 || p.sweep_leaves < 1 || p.sweep_leaves > 32)) return l;
  l.lds = v.sweep ? sweep_lds_bytes(p) : lds_scene ? scene_lds_bytes(p) : 0;
  if (l.lds > kMaxSceneLds) return l;
  l.v = v;
  l.what = Launch::Run;
  return l;
}

// ... and of launch_wavefront_adaptive's (an adaptive round on the wavefront pipeline, kernels/wf_adaptive.h).
// The host does not know how many tiles the round's list holds, so everything is sized for the worst case,
// every tile live: blocks_total * 256 pixel slots, the round's batches in chunks of cap / px, a generation
// grid of blocks_total * chunk workgroups and a fold grid of blocks_total.  The trace, tail and shading
// kernels are pick_wavefront's, moments on and counters off.
//
// Path numbering inside a chunk of nb batches: path g = (e * 256 + q) * nb + s is sample s of pixel q
// (x = list[e].x + q % 16, y = list[e].y + q / 16) of live entry e, and exists iff e < *n_live and the pixel
// lies inside the frame.  256 * nb is a multiple of 256, so generation workgroup `block` lies inside entry
// block / nb.  g is 64-bit: a grid of up to 2^31 - 1 workgroups numbers paths far past 2^31 (a chunk's never
// are: px * chunk <= cap <= 2^31 - 1, which is what keeps the path ids of the lists in an int).
struct WfAdaptivePath {
  uint32_t entry, q, s;   // live entry, pixel within its 16x16 tile, sample within the chunk
  long long g;            // the path: ((long long)entry * 256 + q) * nb + s
};
__host__ __device__ inline long long wf_adaptive_index(long long entry, int q, uint32_t s, uint32_t nb) {
  return (entry * 256 + q) * (long long)nb + s;
}
// Thread `tid` of generation workgroup `block`, nb in 1..65536 (so 256 * nb fits 32 bits with room).
__host__ __device__ inline WfAdaptivePath wf_adaptive_path(uint32_t block, uint32_t tid, uint32_t nb) {
  WfAdaptivePath a;
  a.entry = block / nb;                                    // workgroup-uniform
  const uint32_t t = (block - a.entry * nb) * 256u + tid;   // the path within the entry's 256 * nb
  a.q = t / nb;
  a.s = t - a.q * nb;
  a.g = (long long)block * 256 + tid;
  return a;
}
struct WfAdaptiveLaunch {
  Launch what = Launch::Refused;
  long long px = 0;          // pixel slots: every tile's
  uint32_t chunk = 0;        // batches per chunk
  long long gen_grid = 0;    // wf_gen_adaptive_kernel's workgroups for a full chunk (a shorter last one: blocks * nb)
  long long fold_grid = 0;   // wf_fold_adaptive_kernel's
  size_t lds_trace = 0;      // the trace kernel's dynamic LDS bytes
  WfPick k = {};
};
// cap: WfBuffers::cap.  p.first_batch / p.n_batches: the round's, the same for every live tile.
inline WfAdaptiveLaunch plan_wavefront_adaptive(const RenderParams& p, long long cap, bool lds_scene, int group4_tris) {
  WfAdaptiveLaunch l;
  if (!spl_valid(p.spl) || !p.moments || p.pack_out || p.items || p.mix || p.nranks != 1) return l;
  if (p.n_batches > 65536u) return l;   // pt_adaptive_params' bound, wf_adaptive_path's
  if (p.blocks_total <= 0 || p.n_batches == 0) {
    l.what = Launch::Nothing;
    return l;
  }
  l.px = (long long)p.blocks_total * 256;
  if (l.px > cap || cap > 0x7fffffffll) return l;
  const size_t lds = lds_scene ? scene_lds_bytes(p) : 0;
  if (lds > kMaxSceneLds) return l;
  const WfPick k = pick_wavefront(lds_scene, p.wide != nullptr, p.wide_qn != 0, false, p.exit_skip != 0, true,
                                  p.wf_tail > 0, p.n_tris < group4_tris);
  if (!k.ok) return l;
  if (k.wide && p.wide_ovf_lanes < 256) return l;   // every lane needs its overflow stack area
  l.chunk = (uint32_t)(cap / l.px < (long long)p.n_batches ? cap / l.px : (long long)p.n_batches);
  l.gen_grid = (long long)p.blocks_total * l.chunk;   // <= cap / 256
  l.fold_grid = p.blocks_total;
  l.lds_trace = k.wide ? 0 : lds;
  l.k = k;
  l.what = Launch::Run;
  return l;
}

// Every listed instantiation is one the picks above can return, and they return no other.
template <class V, size_t N>
constexpr bool all_met(const V (&)[N], unsigned met) { return met == (1u << N) - 1u; }
constexpr bool variant_lists_exact() {
  unsigned r = 0, t = 0, w = 0, s = 0, x = 0;   // the listed variants met, as bit sets
  bool ok = true;
  auto mark = [&ok](unsigned& met, int i) {
    ok = ok && i >= 0;
    met |= i >= 0 ? 1u << i : 0u;
  };
  for (int f = 0; f < 256; ++f) {
    const auto bit = [f](int i) { return ((f >> i) & 1) != 0; };
    const RenderPick a = pick_render(bit(0), bit(1), bit(2), (f >> 6) & 3, bit(3), bit(4), bit(5));
    if (a.ok) mark(r, variant_index(kRenderVariants, a.v));
    const WfPick b = pick_wavefront(bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7));
    if (!b.ok) continue;
    if (b.wide)
      mark(w, variant_index(kWfWideVariants, b.wide_trace));
    else
      mark(t, variant_index(kWfTraceVariants, b.trace));
    mark(s, variant_index(kWfShadeVariants, b.shade));
    if (b.tail) mark(x, variant_index(kWfTailVariants, b.tail_v));
  }
  return ok && all_met(kRenderVariants, r) && all_met(kWfTraceVariants, t) && all_met(kWfWideVariants, w) &&
         all_met(kWfShadeVariants, s) && all_met(kWfTailVariants, x);
}
static_assert(variant_lists_exact(), "the variant lists and the picks disagree");
constexpr bool adaptive_list_exact() {
  unsigned met = 0;
  bool ok = true;
  for (int f = 0; f < 16; ++f) {
    const int i = variant_index(kAdaptiveVariants, pick_adaptive((f & 1) != 0, (f >> 2) & 3, (f & 2) != 0));
    ok = ok && i >= 0;
    met |= i >= 0 ? 1u << i : 0u;
  }
  return ok && all_met(kAdaptiveVariants, met);
}
static_assert(adaptive_list_exact(), "the adaptive variant list and its pick disagree");

// ... and of launch_rays' (batched ray queries, kernels/rays.h).  A scene whose wide walk is set up
// (p.wide) is walked by rays_wide_kernel<KIND, QN, REFILL>, then once more by rays_exact_kernel<KIND, false>
// over the rays that kernel marked; any other scene by rays_exact_kernel<KIND, LDS> alone.
struct RaysExactVariant { int kind; bool lds; };          // rays_exact_kernel<KIND, LDS>
struct RaysWideVariant { int kind; bool qn, refill; };    // rays_wide_kernel<KIND, QN, REFILL>
constexpr bool operator==(const RaysExactVariant& a, const RaysExactVariant& b) {
  return a.kind == b.kind && a.lds == b.lds;
}
constexpr bool operator==(const RaysWideVariant& a, const RaysWideVariant& b) {
  return a.kind == b.kind && a.qn == b.qn && a.refill == b.refill;
}
#define PT_RAYS_EXACT_VARIANTS(X) X(0, false) X(0, true) X(1, false) X(1, true)
#define PT_RAYS_WIDE_VARIANTS(X)                                                                    \
  X(0, true, true) X(0, true, false) X(0, false, true) X(0, false, false) X(1, true, true)         \
  X(1, true, false) X(1, false, true) X(1, false, false)
constexpr long long kRaysMax = 0x7fffffffll - 255;   // rays a call takes: indices and the ray counter stay in 32 bits
constexpr long long kRaysLdsGrid = 2048;             // workgroups of the LDS-staged exact kernel: each stages the scene once
struct RaysLaunch {
  Launch what = Launch::Refused;
  bool wide = false;           // the wide kernel, then the exact one over its marks
  RaysWideVariant wide_v = {};
  long long grid_wide = 0;
  RaysExactVariant exact_v = {};
  long long grid_exact = 0;    // workgroups of the exact kernel (striding over the batch)
  size_t lds = 0;              // its dynamic LDS bytes
};
// kind: kRaysClosest / kRaysAny.  refill: PT_OPT_RAYS_REFILL.  wide_blocks: workgroups of the wide kernel
// resident on the device at once (the persistent grid before PT_OPT_WF_GRID and the overflow areas bound it).
inline RaysLaunch plan_rays(const RenderParams& p, int kind, long long n, bool lds_scene, bool refill,
                            long long wide_blocks) {
  RaysLaunch l;
  if ((kind != kRaysClosest && kind != kRaysAny) || n < 0 || n > kRaysMax) return l;
  if (n == 0) {
    l.what = Launch::Nothing;
    return l;
  }
  const long long blocks = (n + 255) / 256;
  l.wide = p.wide != nullptr;
  if (l.wide) {
    if (p.wide_ovf_lanes < 256 || wide_blocks < 1) return l;   // every lane needs its overflow stack area
    long long g = wide_blocks;
    if (p.wf_grid > 0 && p.wf_grid < 100) g = g * p.wf_grid / 100 > 1 ? g * p.wf_grid / 100 : 1;
    if (g > p.wide_ovf_lanes / 256) g = p.wide_ovf_lanes / 256;
    l.grid_wide = g < blocks ? g : blocks;
    l.wide_v = {kind, p.wide_qn != 0, refill};
    l.exact_v = {kind, false};
    l.grid_exact = blocks;
  } else {
    l.lds = lds_scene ? scene_lds_bytes(p) : 0;
    if (l.lds > kMaxSceneLds) return l;
    l.exact_v = {kind, lds_scene};
    l.grid_exact = lds_scene && blocks > kRaysLdsGrid ? kRaysLdsGrid : blocks;
  }
  l.what = Launch::Run;
  return l;
}

// ... and of launch_radiance's (radiance queries, kernels/radiance.h): one chunk of n_queries whole queries of
// n_samples samples each.  wf false: radiance_kernel<LDS, SWEEP, EXIT>, render_adaptive_kernel's variants
// under the same pick (pick_adaptive: the plain kernels, no stats, counters or packed output), one workgroup
// per 256 paths.  wf true: wf_gen_rays_kernel, then the ray rounds of pick_wavefront's kernels (counters and
// moments off) over path buffers of `cap` paths.  Both end with radiance_fold_kernel, one lane per query.
typedef AdaptiveVariant RadianceVariant;   // radiance_kernel<LDS, SWEEP, EXIT>
#define PT_RADIANCE_VARIANTS(X) PT_ADAPTIVE_VARIANTS(X)
constexpr uint32_t kRadianceMaxSamples = 65536;
constexpr long long kRadianceMaxPaths = 0x7fffffffll - 255;   // paths of one chunk: a path index stays an int
struct RadianceLaunch {
  Launch what = Launch::Refused;
  bool wf = false;
  long long paths = 0;       // n_queries * n_samples
  long long grid = 0;        // radiance_kernel's or wf_gen_rays_kernel's workgroups
  long long fold_grid = 0;   // radiance_fold_kernel's
  size_t lds = 0;            // dynamic LDS bytes: radiance_kernel's, or the threaded trace kernel's
  RadianceVariant v = {};    // !wf
  WfPick k = {};             // wf
};
inline RadianceLaunch plan_radiance(const RenderParams& p, bool wf, bool lds_scene, long long n_queries,
                                    uint32_t n_samples, long long cap, int group4_tris) {
  RadianceLaunch l;
  l.wf = wf;
  if (n_samples < 1u || n_samples > kRadianceMaxSamples || n_queries < 0) return l;
  if (n_queries > kRadianceMaxPaths / (long long)n_samples) return l;
  l.paths = n_queries * (long long)n_samples;
  if (l.paths == 0) {
    l.what = Launch::Nothing;
    return l;
  }
  l.grid = (l.paths + 255) / 256;
  l.fold_grid = (n_queries + 255) / 256;
  const size_t lds = lds_scene ? scene_lds_bytes(p) : 0;
  if (wf) {
    if (l.paths > cap || cap > 0x7fffffffll || lds > kMaxSceneLds) return l;
    const WfPick k = pick_wavefront(lds_scene, p.wide != nullptr, p.wide_qn != 0, false, p.exit_skip != 0, false,
                                    p.wf_tail > 0, p.n_tris < group4_tris);
    if (!k.ok) return l;
    if (k.wide && p.wide_ovf_lanes < 256) return l;   // every lane needs its overflow stack area
    l.lds = k.wide ? 0 : lds;
    l.k = k;
  } else {
    const int table = !p.sweep ? 0 : p.sweep_cube ? 3 : p.sweep_hull ? 2 : 1;
    const RadianceVariant v = pick_adaptive(lds_scene, table, p.exit_skip != 0);
    if (v.sweep && (p.sweep_boxes < 1 || p.sweep_boxes > 64 || p.sweep_leaves < 1 || p.sweep_leaves > 32)) return l;
    l.lds = v.sweep ? sweep_lds_bytes(p) : lds;
    if (l.lds > kMaxSceneLds) return l;
    l.v = v;
  }
  l.what = Launch::Run;
  return l;
}
#pragma GCC visibility pop

}  // namespace ptd
