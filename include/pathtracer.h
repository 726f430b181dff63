/*
 * pathtracer.h — C ABI of the MI355X-native path-tracing pixel kernel.
 *
 * This is the drop-in boundary.  The reference has no plugin/operator API:
 * its seam is the Vulkan compute interface that VulkanRayTracer builds and
 * drives (src/Vulkan/VulkanRayTracer.cpp) for the shader
 * src/shaders/raytrace_comp.comp.  Every entry point below replaces one piece
 * of that seam; the comment on each cites what it replaces.  A maintainer
 * swaps the Vulkan descriptor/dispatch code for these calls.
 *
 * Conventions (inherited from the reference):
 *   - every call returns int status: PT_OK (0) or a negative PT_ERR_*;
 *     pt_last_error() describes the last failure on the calling thread.
 *     Nothing throws across the ABI.
 *   - the caller keeps ownership of every host array; uploads copy.
 *   - the accumulation buffer is device-resident (RGBA32F, row-major,
 *     pixel (x,y) at index y*W+x) until read back.
 *   - one context per GPU, driven from one thread.  Calls are ordered on the
 *     context's HIP stream; pt_dispatch/pt_render return once the work is
 *     enqueued, pt_read_accum/pt_synchronize wait for it (the reference blocks
 *     on a fence after every dispatch, VulkanCommandBuffer.cpp:140).
 */
#ifndef PATHTRACER_H_
#define PATHTRACER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  2 (round 5): pt_group_check, pt_dist_info and
 * PT_OPT_GROUP_CHECK added; option values removed since 1 now return
 * PT_ERR_UNSUPPORTED: PT_OPT_KERNEL 2, PT_OPT_SM_BATCH, PT_OPT_PAIRS 1,
 * PT_OPT_WIDE_NODE 80 (kernels measured slower on every scene).
 * 3 (round 6): pt_mixed_info and PT_OPT_MIXED_LANES added; defaults changed:
 * PT_OPT_LAUNCH_TIMING 0 (was 1), PT_OPT_ITEM_ORDER -1 auto (was 1);
 * pt_group_check state 2 (probe failed).
 * Still 3, additions only: the guide image and the a-trous denoiser
 * (pt_denoise_params, pt_denoise_default_params, pt_guide_ray,
 * pt_render_guide, pt_guide_device_ptr, pt_read_guide, pt_denoise,
 * pt_read_denoised, pt_denoise_host, PT_OPT_DENOISE_LDS); the sweep walk of
 * tiny scenes (pt_sweep_info, PT_OPT_SMALL_SWEEP); the tight cull rectangles
 * and the sweep's hull faces (pt_primary_cull_rects_r, PT_OPT_CULL_TIGHT,
 * PT_OPT_SWEEP_HULL); the per-pixel luminance moments and the
 * variance-guided filter (PT_OPT_MOMENTS, pt_moments_device_ptr,
 * pt_read_moments, pt_denoise_var_params, pt_denoise_var_default_params,
 * pt_denoise_var, pt_denoise_var_host); the exit skip (PT_OPT_EXIT_SKIP); the
 * seed base and temporal reprojection (PT_OPT_SEED_BASE, pt_temporal_params,
 * pt_reproject_images, pt_temporal_default_params, pt_reproject,
 * pt_reproject_host, pt_temporal_advance, pt_temporal_reset, pt_temporal_info,
 * pt_temporal_device_ptr, pt_read_temporal, pt_temporal_denoise,
 * pt_denoise_var_plane_host); the spatial variance estimate of short histories
 * (pt_spatial_var_params, pt_spatial_var_default_params,
 * pt_spatial_variance_host, pt_spatial_variance, pt_temporal_denoise_spatial);
 * the straight-line sweep of a cube table (PT_OPT_SWEEP_CUBE, pt_sweep_walk);
 * adaptive sampling (pt_adaptive_params, pt_adaptive_default_params,
 * pt_adaptive_select_host, pt_adaptive_select, pt_adaptive_begin,
 * pt_adaptive_advance, pt_adaptive_info, pt_adaptive_read_counts,
 * pt_adaptive_read_live, pt_adaptive_device_ptr, pt_adaptive_denoise); the
 * display transform (pt_display_params, pt_display_default_params, pt_display,
 * pt_display_device_ptr, pt_read_display, pt_display_exposure, pt_display_reset,
 * pt_display_readback_begin, pt_display_readback_end, pt_display_host,
 * pt_write_png8); batched ray queries (pt_ray, pt_hit, PT_RAYS_CLOSEST,
 * PT_RAYS_ANY, pt_trace_rays, pt_trace_rays_sync, pt_trace_rays_host,
 * PT_OPT_RAYS_REFILL); guide-driven upsampling (pt_upsample_params,
 * pt_upsample_default_params, pt_upsample_host, pt_upsample_images,
 * pt_upsample, pt_upsampled_device_ptr, pt_read_upsampled,
 * pt_upsample_guide_device_ptr, pt_upsample_info, pt_upsample_display,
 * pt_display_upsampled_device_ptr, pt_read_display_upsampled); radiance
 * queries (pt_radiance_params, pt_radiance_default_params, pt_trace_radiance,
 * pt_trace_radiance_sync, pt_trace_radiance_host, pt_camera_rays,
 * pt_camera_rays_host, PT_OPT_RADIANCE_CHUNK). */
#define PT_ABI_VERSION 3

enum {
  PT_OK = 0,
  PT_ERR_INVALID = -1,     /* bad argument / state */
  PT_ERR_HIP = -2,         /* HIP runtime failure */
  PT_ERR_SCENE = -3,       /* malformed scene / BVH */
  PT_ERR_IO = -4,          /* file not found / parse error */
  PT_ERR_UNSUPPORTED = -5  /* valid input this build does not handle */
};

/* BVHNode — src/BoundingVolumeHierarchy.h:8-13, std430 stride 32 B.
 * min_bounds.w = left child or -1 (leaf); max_bounds.w = right child or the
 * leaf's triangle index.  Indices are floats (reference) unless
 * PT_NODES_INT_BITS is passed, in which case they are int32 bit patterns. */
typedef struct pt_bvh_node {
  float min_bounds[4];
  float max_bounds[4];
} pt_bvh_node;

/* AreaLightData — src/Light.h:6-12, 64 B. */
typedef struct pt_area_light {
  float position[4];
  float normal[4];
  float intensity[4];
  float size[4];
} pt_area_light;

/* Tunables the reference hard-codes (raytrace_comp.comp:304,373). */
typedef struct pt_params {
  int max_depth;    /* MAX_DEPTH, reference 4 */
  int sss_bounces;  /* SSS_MAX_BOUNCES, reference 3 */
} pt_params;

/* Statistics of the reference traversal (exhaustive DFS, raytrace_comp.comp:159-204),
 * accumulated while stats mode is on: traceRay calls, BVH nodes visited,
 * leaf triangle tests, pixel-samples. */
typedef struct pt_stats {
  uint64_t rays;
  uint64_t nodes;
  uint64_t leaf_tests;
  uint64_t samples;
} pt_stats;

/* Work the fast kernels actually did while PT_OPT_COUNT_TRACED is on (they
 * skip work the reference does without changing a bit of the output: culled
 * primary rays, shadow rays whose answer cannot change the image, the
 * repeated light pre-pass ray, implied-hit nodes, leaf tests after an
 * occluder): closest-hit and shadow walks started, BVH nodes visited,
 * triangle tests, primary rays generated.  Reset by pt_reset_stats. */
typedef struct pt_traced {
  uint64_t closest_walks;
  uint64_t shadow_walks;
  uint64_t nodes;
  uint64_t tri_tests;
  uint64_t primaries;
} pt_traced;

typedef struct pt_context pt_context;

/* upload flags */
#define PT_NODES_INT_BITS 0x1u

/* ---- lifetime ---------------------------------------------------------- */
int pt_abi_version(void);
const char* pt_last_error(void);
/* Replaces VulkanWindow's device/queue selection (VulkanWindow.cpp:106-174)
 * and VulkanRayTracer::initComputePipeline's pipeline creation (:624-672). */
int pt_create(int device_ordinal, pt_context** out);
/* One context over n devices of this process (SURVEY.md §8b create(device
 * ordinals[], n)): the reference's single host thread (VulkanRenderer.cpp:
 * 643-647, mainLoop VulkanRayTracer.cpp:717-865) drives all of them through
 * the calls below exactly as it drives one.  Member r renders the 16x16
 * screen tiles of rank r of an n-way pt_set_partition; the frame lives in
 * device memory of device_ordinals[0] (pt_accum_device_ptr), where pt_read_accum,
 * pt_readback_* and pt_synchronize see every member's tiles, bit-identical to
 * a single-GPU render.  Members store their tiles into that frame directly
 * over xGMI (peer access), or -- when a member cannot map it, or with
 * PT_OPT_GROUP_EXCHANGE 1 -- ship them as packed tiles copied to the first
 * device.  Before peer stores carry a frame on members of distinct devices,
 * a probe frame checks them bit for bit against the packed copies and falls
 * back to the copies on any difference (PT_OPT_GROUP_CHECK, pt_group_check).
 * UNVERIFIED on hardware: members on distinct devices have not run in this
 * build's tests (one-GPU boxes); every group test so far put its members on
 * one device, where the bit identity is tested.  An ordinal may repeat (several members on one device: tests).
 * With three or more members, members 1..n-1 enqueue their launches from
 * threads of their own (environment PT_GROUP_THREADS=0: all on the calling
 * thread), so a render costs the caller about one member's host time.
 * Calls on a member's share (pt_set_partition*, pt_tiles_*, pt_items_*,
 * pt_render_packed, pt_dist_*) return PT_ERR_UNSUPPORTED on such a context;
 * the launch-timing calls report the first device's launches.  pt_destroy
 * frees it. */
int pt_create_multi(const int* device_ordinals, int n, pt_context** out);
/* Devices of a context (1 and its ordinal for a pt_create context) and
 * whether its members store their tiles straight into the frame (1) or ship
 * packed tiles (0). */
int pt_group_info(pt_context* ctx, int* n_devices, int* devices, int max_devices, int* peer_stores);
/* The peer-store check of a multi-device context (PT_OPT_GROUP_CHECK):
 * *state -2 armed (runs on the next render), -1 not run (members on one
 * device, staged exchange in force, or a pt_create context), 0 the probe
 * frames matched bit for bit (peer stores in force), 1 they differed (the
 * staged exchange is in force from then on), 2 the peer-store probe failed
 * (a HIP error; staged exchange from then on, the render goes on); the probe
 * frames' wall times.  The probe is read back the way a frame is consumed:
 * on the first device's stream, behind its wait for every member's
 * completion event, with no host synchronisation of the members before it.
 * The check is meant to catch a cross-device visibility failure of peer
 * stores at run time; it has not yet run on members of distinct devices
 * (every test so far ran its members on one device), so whether it does is
 * unverified. */
int pt_group_check(pt_context* ctx, int* state, float* ms_peer, float* ms_staged);
int pt_destroy(pt_context* ctx);
/* Launch on a caller-owned hipStream_t (e.g. a torch.cuda.Stream's handle);
 * NULL returns to the context's own stream — so the legacy default stream
 * (handle 0) cannot be selected: share a created stream instead. */
int pt_set_stream(pt_context* ctx, void* hip_stream);
int pt_synchronize(pt_context* ctx);

/* ---- scene upload (VulkanRayTracer.cpp:100-311, bindings 1,2,3,6,7) ---- */
/* vertices: float[3V] (binding 1); indices: uint[3T] in BVH-leaf order
 * (binding 2); nodes: BVHNode[2T-1] (binding 3); uvs (binding 6) and
 * mat_indices (binding 7) are accepted for interface parity and validated but
 * do not affect the output (raytrace_comp.comp:150-154,192 are dead). */
int pt_upload_scene(pt_context* ctx,
                    const float* vertices, size_t n_vertex_floats,
                    const uint32_t* indices, size_t n_indices,
                    const pt_bvh_node* nodes, size_t n_nodes,
                    const float* uvs, size_t n_uv_floats,
                    const uint32_t* mat_indices, size_t n_mat,
                    uint32_t flags);
/* binding 5 (VulkanRayTracer.cpp:165-176) */
int pt_upload_lights(pt_context* ctx, const pt_area_light* lights, size_t n_lights);
/* binding 4: std140 CameraBuffer — pos@0, dir@16, up@32, fov.x@48
 * (raytrace_comp.comp:67-73; written at VulkanRayTracer.cpp:761-764). */
int pt_set_camera(pt_context* ctx, const float camera_ubo[16]);
int pt_set_params(pt_context* ctx, const pt_params* params);

/* ---- accumulation image (binding 0, VulkanRayTracer.cpp:317-320) ------- */
/* Allocate (or reuse) a W x H RGBA32F buffer and zero it.  The reference
 * never clears its image (VulkanImage.cpp:71); batch 0 multiplies prev by 0. */
int pt_resize_and_clear(pt_context* ctx, int width, int height);
/* Render into caller-owned device memory of W*H*16 bytes instead (not
 * cleared; call pt_clear_accum). */
int pt_bind_accum(pt_context* ctx, void* device_ptr, int width, int height);
int pt_clear_accum(pt_context* ctx);
void* pt_accum_device_ptr(pt_context* ctx);
int pt_read_accum(pt_context* ctx, float* rgba, size_t n_floats);

/* ---- the hot path ------------------------------------------------------ */
/* One 1-spp accumulation pass with push constant sample_batch
 * (VulkanRayTracer.cpp:803-813 vkCmdPushConstants + vkCmdDispatch). */
int pt_dispatch(pt_context* ctx, uint32_t sample_batch);
/* n_batches sequential passes first_batch..first_batch+n-1 fused into one
 * launch; bit-identical to that many pt_dispatch calls. */
int pt_render(pt_context* ctx, uint32_t first_batch, uint32_t n_batches);

/* ---- progressive loop (VulkanRayTracer::mainLoop, :717-865) ------------ */
/* Sets the camera; if any of its 16 floats differs from the last one given
 * here, the sample counter restarts at 0 (:739-754 — batch 0 weights the old
 * image by 0, so no clear is needed).  *reset (optional) reports it. */
int pt_progressive_camera(pt_context* ctx, const float camera_ubo[16], int* reset);
/* Enqueues min(max_new, limit - counter) further batches as one fused launch
 * (the reference renders up to limit = 1024, :719) and advances the counter;
 * *first and *count (optional) report what was enqueued.  Bit-identical to
 * that many pt_dispatch calls. */
int pt_progressive_advance(pt_context* ctx, uint32_t max_new, uint32_t limit, uint32_t* first, uint32_t* count);
/* Asynchronous double-buffered readback (replaces the per-batch fence waits
 * and copyStorageImage, :826-846): begin snapshots the image as of the work
 * enqueued so far and copies it to pinned host memory on a second stream;
 * end waits for that copy and writes W*H*4 floats.  Two readbacks may be in
 * flight; a third begin recycles the oldest unclaimed one. */
int pt_readback_begin(pt_context* ctx, int* ticket);
int pt_readback_end(pt_context* ctx, int ticket, float* rgba, size_t n_floats);

/* ---- first-hit guide image and edge-avoiding a-trous denoiser ---------- */
/* Downstream of pt_render: nothing in the reference corresponds to it (its
 * image leaves as it is, VulkanRayTracer.cpp:826-846).  Single-GPU contexts
 * only: on a pt_create_multi context every call below that takes a context
 * returns PT_ERR_UNSUPPORTED (pt_guide_device_ptr: null).
 *
 * The guide image holds, per pixel, float4 {n.x, n.y, n.z, t}: normal and
 * distance of the first hit of the pixel's centre ray, {0, 0, 0, 1e30} for a
 * miss (HitInfo's initial value).  The ray is main()'s without its random
 * draws (raytrace_comp.comp:430-432, :458): origin = camera position,
 *   ndcX = ((2 * float(x)) / float(W)) - 1, ndcY likewise, aspect = float(W) / float(H),
 *   dir  = normalize((cameraDir + (-right) * ((ndcX * tanFov) * aspect)) - up * (ndcY * tanFov)),
 * traced by one traceRay (:159-204) -- the same hit bit for bit on every walk
 * the library has.  It is a pinhole ray: the shader's depth-of-field blur
 * (aperture 0.02, focal distance 3) makes the guide's edges slightly sharper
 * than the image's.  The image covers every pixel, whatever the partition.
 *
 * The filter (Dammertz, Sewtz, Hanika, Lensch: "Edge-avoiding A-trous wavelet
 * transform for fast global illumination filtering", HPG 2010), restated so
 * that it is bit-reproducible.  Pass i = 0 .. iterations-1 has tap spacing
 * s = 1 << i and sc = sigma_color * 2^-i (exact); sn = sigma_normal, sz =
 * sigma_depth.  For pixel p with colour c_p (the pass's input) and guide g_p,
 * over the 25 taps q = p + s * (dx, dy), dy = -2..2 outer, dx = -2..2 inner
 * (the summation order), those outside the frame skipped:
 *   h   = k[|dx|] * k[|dy|],  k = {3/8, 1/4, 1/16}
 *   d2c = (dr*dr + dg*dg) + db*db            (rgb of c_p - c_q)
 *   d2n = (dnx*dnx + dny*dny) + dnz*dnz      (normals of g_p - g_q)
 *   dz  = t_p - t_q
 *   w   = h * exp(-((d2c / (sc*sc) + d2n / (sn*sn)) + (dz*dz) / (sz*sz)))
 *   sum_c += w * c_q.rgb;  sum_w += w
 * and out.rgb = sum_c / sum_w, out.a = c_p.a.  exp is the library's pinned
 * fp32 exp (pt_selftest_math fn 1), divisions are IEEE, nothing is fused.  A
 * hit next to a miss has dz*dz = inf, hence w = 0; two misses have dz = 0.
 * The centre tap weighs 9/64, so sum_w > 0 for finite input.  The passes
 * ping-pong between two library-owned images; the source is only read.
 *
 * Non-finite and extreme input.  "The same bits" between a kernel and its host
 * function, here and for every function further down, means: a NaN where the
 * other has a NaN (its sign and payload are the platform's), every other float
 * the same bits, the sign of a zero included.  That holds for any input bits:
 * NaN, infinities, negative and subnormal values, magnitudes whose squares
 * overflow.  No filter skips a tap of weight 0, so a tap on an infinite colour
 * adds 0 * inf = NaN: one infinite pixel turns the 25 pixels that tap it into
 * NaN in one pass, the (4 (2^k - 1) + 1)^2 block around it in k passes.  A range
 * test written x < y or !(x > y) is false, respectively true, for a NaN, as
 * written.  fmax(0, x), the clamp of a variance, is x where x > 0 and +0
 * otherwise -- for a NaN and for -0 too; every other fmin / fmax is minNum /
 * maxNum (a NaN operand yields the other one) and never sees two zeros.
 *
 * Defaults (pt_denoise_default_params): 5 iterations, sigma_color 16,
 * sigma_normal 0.35, sigma_depth 0.25, chosen on two 256x256 8-spp frames
 * against 256-spp frames of the same view (mean squared rgb error, raw ->
 * denoised): box.obj, default camera, 1.1497e-01 -> 2.0946e-02; the displaced
 * sphere (5,120 triangles) from (3, 2, 4), 5.3595e-02 -> 2.5855e-02.  The
 * image is linear radiance with the light (intensity 10) in view and 8-spp
 * pixel noise of order 1, hence the large sigma_color; a tone-mapped or
 * darker input wants a smaller one (DESIGN.md §9 has the search). */
typedef struct pt_denoise_params {
  int iterations;      /* 1 to 6 */
  float sigma_color;   /* all three finite and > 0, their squares (and that of */
  float sigma_normal;  /* sigma_color * 2^-(iterations-1)) finite and non-zero */
  float sigma_depth;
} pt_denoise_params;
int pt_denoise_default_params(pt_denoise_params* out);
/* The guide ray of pixel (x, y) of a W x H frame: origin and direction.
 * Pure host function; the device computes the same bits. */
int pt_guide_ray(const float camera_ubo[16], int width, int height, int x, int y, float o3[3], float d3[3]);
/* Enqueues the guide image of the current scene, camera and frame size into
 * a library-owned W x H float4 image (PT_ERR_INVALID without a scene, a
 * camera or an accumulation image).  A scene with a culled wide tree
 * (pt_wide_info, PT_OPT_WIDE not 0) is walked by it, rays with a zero
 * direction component by the exact walk; other scenes by the exact walk, from
 * LDS when PT_OPT_SCENE_IN_LDS puts them there. */
int pt_render_guide(pt_context* ctx);
/* The guide image in device memory, or null when there is none for the
 * current inputs: a scene upload, a camera that differs (pt_set_camera,
 * pt_progressive_camera) and a change of size (pt_resize_and_clear,
 * pt_bind_accum) invalidate it. */
void* pt_guide_device_ptr(pt_context* ctx);
/* Waits for the guide and copies its W*H*4 floats. */
int pt_read_guide(pt_context* ctx, float* out, size_t n_floats);
/* Enqueues the filter, one launch per pass, on the context's stream, after
 * rendering the guide if there is none for the current inputs.  params null:
 * the defaults.  src_device null: the accumulation image, else W*H float4 in
 * device memory (16-B aligned).  dst_device null: a library-owned image
 * (pt_read_denoised), else W*H float4 in device memory, distinct from the
 * source.  PT_ERR_INVALID for bad parameters, without a scene, a camera or an
 * accumulation image (its size is the frame's). */
int pt_denoise(pt_context* ctx, const pt_denoise_params* params, const void* src_device, void* dst_device);
/* Waits for the last pt_denoise into the library-owned image and copies it. */
int pt_read_denoised(pt_context* ctx, float* rgba, size_t n_floats);
/* The same filter on the host (the same header code the kernels compile):
 * rgba, guide and out hold W*H*4 floats; params null: the defaults.  Pure
 * host function; bit-identical to pt_denoise. */
int pt_denoise_host(const float* rgba, const float* guide, int width, int height, const pt_denoise_params* params,
                    float* out);

/* ---- per-pixel luminance moments and the variance-guided filter --------
 * With PT_OPT_MOMENTS 1 every pt_dispatch, pt_render and
 * pt_progressive_advance also folds, per pixel, into a library-owned W x H
 * image of float2 {m1, m2}:
 *   L  = (0.2126f * r + 0.7152f * g) + 0.0722f * b   rgb of the sample's colour
 *   m1 = (m1 * float(batch) + L)       / float(batch + 1)
 *   m2 = (m2 * float(batch) + (L * L)) / float(batch + 1)
 * the accumulator's own fold, in batch order, IEEE division, nothing fused.
 * A culled pixel and a sample PT_OPT_CULL_TIGHT skips have L = +0.  After a
 * render that starts at batch 0 every pixel of the frame holds the value of
 * this definition.  pt_clear_accum, pt_resize_and_clear and pt_bind_accum
 * zero the image.  The context tracks the consecutive batches 0..n-1 the image
 * holds: a render with moments on whose first_batch is neither 0 nor n, and a
 * render with moments off that changes the accumulator, make the moments
 * invalid until the next render from batch 0 with moments on.
 * PT_ERR_UNSUPPORTED with the option on: multi-device contexts, a partition of
 * more than one rank, pt_render_packed, pt_dist_run, stats mode,
 * PT_OPT_COUNT_TRACED. */
/* The moments image in device memory; null when off or invalid. */
void* pt_moments_device_ptr(pt_context* ctx);
/* Waits for the moments and copies W*H*2 floats; *n_samples (may be null)
 * receives n, or 0 when the image is invalid (its content is then whatever
 * the renders since the last clear folded).  PT_ERR_INVALID with the option
 * off or before the first render with it. */
int pt_read_moments(pt_context* ctx, float* out, size_t n_floats, uint32_t* n_samples);
/* The a-trous filter above with its colour edge-stop driven by each pixel's
 * variance of the mean (SVGF): strong where the estimate is noisy, fading out
 * as the render converges.  From the accumulation image c, its moments of n
 * samples and the guide (n.xyz, t), lum() being the L above:
 *   var0_p = fmax(0, m2_p - m1_p * m1_p) / float(n - 1)
 *   pass i = 0 .. iterations-1, s = 1 << i, on colour c and variance v (v = var0 in pass 0):
 *     gv_p  = (sum of (g[|dx|] * g[|dy|]) * v_q) / (sum of g[|dx|] * g[|dy|])
 *             over q = p + (dx, dy), dy = -1..1 outer, dx = -1..1 inner, spacing 1,
 *             taps outside the frame skipped, g = {1/2, 1/4}
 *     den_p = sigma_lum * sqrt(gv_p) + 1e-6f
 *     over the 25 taps q = p + s * (dx, dy), dy outer, dx inner, outside skipped
 *     (h, d2n, dz, sn2, sz2 as in pt_denoise):
 *       w      = h * exp(-((fabs(lum(c_p) - lum(c_q)) / den_p + d2n / sn2) + (dz * dz) / sz2))
 *       sum_c += w * c_q.rgb;   sum_v += (w * w) * v_q;   sum_w += w
 *     out.rgb = sum_c / sum_w,  out.a = c_p.a,  v_out = sum_v / (sum_w * sum_w)
 * One rounding per written operation; sigma_lum is not scaled per pass.
 * Defaults (pt_denoise_var_default_params): 4 iterations, sigma_lum 1.5,
 * sigma_normal 1, sigma_depth 1: the best point of a grid scored on 8- and
 * 32-spp frames of two scenes against 256 spp. */
typedef struct pt_denoise_var_params {
  int iterations;      /* 1 to 6 */
  float sigma_lum;     /* all three finite and > 0, their squares finite and */
  float sigma_normal;  /* non-zero */
  float sigma_depth;
} pt_denoise_var_params;
int pt_denoise_var_default_params(pt_denoise_var_params* out);
/* Enqueues the filter of the accumulation image with its moments, after
 * rendering the guide if there is none.  dst_device null: the library-owned
 * image pt_read_denoised reads; else W*H float4, 16-B aligned, not the
 * accumulation image.  PT_ERR_INVALID without valid moments, with n < 2, with
 * bad parameters, without a scene, a camera or a frame.  PT_OPT_DENOISE_LDS
 * picks the staged kernels for spacings 1 and 2 as for pt_denoise (same bits). */
int pt_denoise_var(pt_context* ctx, const pt_denoise_var_params* params, void* dst_device);
/* The same filter on the host: rgba, guide and out W*H*4 floats, moments
 * W*H*2, n_samples >= 2.  Pure host function; bit-identical to pt_denoise_var. */
int pt_denoise_var_host(const float* rgba, const float* moments, uint32_t n_samples, const float* guide, int width,
                        int height, const pt_denoise_var_params* params, float* out);
/* The same passes on the host from an explicit variance plane of W*H floats
 * (pass 0's v) instead of moments: pt_denoise_var_host is this function after
 * its own var0.  Pure host function; bit-identical to pt_temporal_denoise. */
int pt_denoise_var_plane_host(const float* rgba, const float* variance, const float* guide, int width, int height,
                              const pt_denoise_var_params* params, float* out);

/* ---- temporal reprojection: frame history across camera moves ----------
 * SVGF's first stage (Schied et al., HPG 2017).  pt_progressive_camera throws
 * the image away when the camera changes, as the reference's mainLoop does;
 * the calls below carry it over instead: the first hit of each pixel of the
 * new frame (its guide) is projected into the previous camera, the previous
 * result is read there through four bilinear taps that pass a depth and a
 * normal test against the previous guide, and the new frame is blended in by
 * sample counts.  Single-GPU contexts only (PT_ERR_UNSUPPORTED otherwise).
 *
 * The statement, shared by the kernel and the host function (every operation
 * rounds once, divisions are IEEE, nothing is fused; cam_basis is the camera
 * frame of the guide ray above: right = normalize(cross(dir, -up)), up' =
 * normalize(cross(right, dir)), tan_fov = tan(radians(fov / 2)); guide_dir is
 * the guide ray's direction).  Per pixel p = (x, y) of a W x H frame:
 *   inputs   c (float4), m (float2 {m1,m2}), n >= 1: the new frame, its moments, its sample count
 *            g (float4 {n.xyz, t}): the new camera's guide;   B = cam_basis(cam_cur), Bp = cam_basis(cam_prev)
 *            hc, hm, hl (float, samples; 0 = none), hg: the history's colour, moments, length and guide
 *   no history for p (out = c, out_m = m, out_len = float(n)) if any "else none" below applies
 *     t = g_p.w;  if !(t < 1e30f) none                                   (a miss)
 *     P = B.pos + guide_dir(B, W, H, x, y) * t
 *     v = P - Bp.pos;  z = dot(v, Bp.dir);  if !(z > 0) none
 *     aspect = float(W) / float(H)
 *     sx = dot(v, -Bp.right) / (z * (Bp.tan_fov * aspect));   sy = dot(v, -Bp.up) / (z * Bp.tan_fov)
 *     fx = ((sx + 1) * float(W)) * 0.5f;   fy = ((sy + 1) * float(H)) * 0.5f
 *     if !(fx > -1 && fx < float(W) && fy > -1 && fy < float(H)) none     (also NaN)
 *     x0f = floor(fx), ax = fx - x0f, x0 = int(x0f);  y likewise;  dexp = length(v)
 *     taps q = (x0 + tx, y0 + ty), ty = 0..1 outer, tx = 0..1 inner, outside the frame skipped:
 *       b = (tx ? ax : 1 - ax) * (ty ? ay : 1 - ay)
 *       valid iff hl_q > 0 && hg_q.w < 1e30f && fabs(hg_q.w - dexp) <= depth_rel * dexp
 *                 && dot(g_p.xyz, hg_q.xyz) >= normal_min
 *       valid: sw += b;  sc.rgb += b * hc_q.rgb;  sm += b * hm_q;  lmin = fmin(lmin, hl_q)
 *     if !(sw > 0) none
 *     h = sc / sw;  h_m = sm / sw;  N = fmin(lmin, float(max_history))
 *     a = fmax(alpha_min, float(n) / (N + float(n)))
 *     out.rgb = h + (c.rgb - h) * a;  out.a = c.a;  out_m = h_m + (m - h_m) * a;  out_len = N + float(n)
 *   always   out_var = fmax(0, out_m.y - out_m.x * out_m.x) / fmax(out_len - 1, 1)
 * t is a distance along a unit ray, so dexp is the distance the previous guide
 * should hold at that point.  The guide ray passes through integer pixel
 * coordinates (ndc = 2x/W - 1): no half-pixel offset appears.
 *
 * Defaults (pt_temporal_default_params): max_history 64, alpha_min 0,
 * normal_min 0.5, depth_rel 0.05.  Ranges: max_history 1..65536, alpha_min in
 * [0, 1], normal_min in [-1, 1], depth_rel finite and > 0; n and n_batches
 * 1..65536, so every length is an exact float.  Null params: the defaults.
 * Anything else: PT_ERR_INVALID. */
typedef struct pt_temporal_params { uint32_t max_history; float alpha_min, normal_min, depth_rel; } pt_temporal_params;
typedef struct pt_reproject_images {            /* device pointers for pt_reproject, host pointers for pt_reproject_host */
  const float *color, *moments, *guide;                                  /* W*H*4, W*H*2, W*H*4 */
  const float *hist_color, *hist_moments, *hist_length, *hist_guide;    /* all four null: no history */
  float *out_color, *out_moments, *out_length, *out_variance;           /* W*H*4, *2, *1, *1; distinct from the inputs */
} pt_reproject_images;
int pt_temporal_default_params(pt_temporal_params* out);
/* Enqueues the statement on the context's stream.  Colours and guides 16-B
 * aligned, moments 8-B, lengths and the variance 4-B; no output may be an
 * input or another output (PT_ERR_INVALID). */
int pt_reproject(pt_context* ctx, const float cam_cur[16], const float cam_prev[16], int width, int height, uint32_t n,
                 const pt_reproject_images* images, const pt_temporal_params* params);
/* The same statement on the host.  Pure host function; the same bits. */
int pt_reproject_host(const float cam_cur[16], const float cam_prev[16], int width, int height, uint32_t n,
                      const pt_reproject_images* images, const pt_temporal_params* params);
/* One frame of the temporal loop, all enqueued and none of it waited for:
 * sets the camera, clears the accumulator, renders batches 0..n_batches-1 with
 * moments at the seed base PT_OPT_SEED_BASE plus the samples rendered since
 * the last reset (mod 2^32) -- the accumulation image and pt_read_moments then
 * hold exactly what pt_render(0, n_batches) at that seed base gives --, renders
 * the guide, and reprojects at the default parameters from the previous call's
 * result, guide and camera into the other of two library-owned image sets
 * (the first frame after a reset: no history).  Needs PT_OPT_MOMENTS 1, a
 * scene, lights and a frame (PT_ERR_INVALID); PT_ERR_UNSUPPORTED where moments
 * are: multi-device contexts, a partition of more than one rank, stats mode,
 * PT_OPT_COUNT_TRACED.  The history is forgotten by pt_temporal_reset,
 * pt_upload_scene, pt_scene_upload, pt_upload_lights, pt_set_params and a
 * change of frame size or of the bound buffer -- never by the camera.
 * pt_render, pt_dispatch and the progressive calls neither use nor disturb
 * it. */
int pt_temporal_advance(pt_context* ctx, const float camera_ubo[16], uint32_t n_batches);
int pt_temporal_reset(pt_context* ctx);
/* Frames and samples (mod 2^32) since the last reset; either may be null. */
int pt_temporal_info(pt_context* ctx, uint32_t* frames, uint32_t* samples);
/* The last result in device memory: which = 0 colour (W*H float4), 1 moments
 * (float2), 2 length in samples (float), 3 variance of the mean (float); null
 * when there is none. */
void* pt_temporal_device_ptr(pt_context* ctx, int which);
/* Waits for the last result and copies it; each pointer may be null. */
int pt_read_temporal(pt_context* ctx, float* rgba, float* moments, float* length);
/* pt_denoise_var's passes on the temporal colour, with the statement's out_var
 * as pass 0's variance and the frame's guide; dst_device as for
 * pt_denoise_var.  PT_ERR_INVALID without a temporal result. */
int pt_temporal_denoise(pt_context* ctx, const pt_denoise_var_params* params, void* dst_device);

/* ---- spatial variance of pixels with too few samples -------------------
 * SVGF's variance estimation stage.  A pixel holding one sample has m2 ==
 * m1 * m1, so the statement's out_var is 0, the filter's den is 1e-6 and every
 * tap of another luminance weighs nothing: at one sample per frame the first
 * frame after a reset, every disoccluded pixel and every pixel entering at the
 * frame edge pass pt_temporal_denoise unfiltered.  Where the history is shorter
 * than `below` samples the variance is therefore estimated from the moments of
 * the neighbourhood under the filter's geometric edge-stops.  The statement,
 * shared by the kernel and the host function (every operation rounds once,
 * divisions are IEEE, nothing is fused, exp is the pinned fp32 exp).  Per pixel
 * p of a W x H frame, from moments m (float2 {m1, m2}), length len (float,
 * >= 1), variance var (float) and guide g (float4 {n.xyz, t}):
 *   if !(len_p < float(below))   out_p = var_p                      (the same bits)
 *   else over q = p + (dx, dy), dy = -radius..radius outer, dx likewise inner,
 *   taps outside the frame skipped, the centre included:
 *     d2n = (dnx*dnx + dny*dny) + dnz*dnz   (normals of g_p - g_q);   dz = g_p.w - g_q.w
 *     w   = exp(-(d2n / (sn*sn) + (dz*dz) / (sz*sz))) * len_q
 *     sw += w;   s1 += w * m_q.x;   s2 += w * m_q.y
 *   M1 = s1 / sw;   M2 = s2 / sw;   out_p = fmax(0, M2 - M1 * M1) / len_p
 * A tap whose guide compares equal to the centre's in all four components (the
 * centre itself, a miss beside a miss) weighs len_q itself: exp(-0) * len_q for
 * a finite guide, and the defined weight where an infinite component would make
 * dz = inf - inf.
 * The centre tap weighs len_p >= 1, so sw > 0 for finite input; a hit next to a
 * miss has dz*dz = inf, hence w = 0; two misses pool their zero moments.  A tap
 * weighs its sample count: M2 - M1 * M1 is the pooled variance of one sample,
 * divided by the pixel's own count.
 *
 * Ranges: below 0..65536 (0 and 1 select no pixel: out = var), radius 1..3,
 * both sigmas finite and > 0 with finite non-zero squares.  Null params: the
 * defaults.  Anything else: PT_ERR_INVALID.
 * Defaults (pt_spatial_var_default_params): below 2, radius 1, sigma_normal 1,
 * sigma_depth 0.5: of a grid over below {2, 3, 4, 8}, radius {1, 2, 3} and both
 * sigmas {0.25, 0.5, 1}, scored on first frames, 60 degree jumps and eighth
 * orbit frames of two scenes at 1 and 2 spp against 256 spp, the best point
 * that leaves no orbit frame worse than pt_temporal_denoise does.  The best
 * point overall, below 8 at the same radius and sigmas, scores 1.3 % better by
 * making 2-spp orbit frames worse; a wider window always scores worse
 * (profiles/spatial_var/grid.json). */
typedef struct pt_spatial_var_params { uint32_t below; int radius; float sigma_normal, sigma_depth; } pt_spatial_var_params;
int pt_spatial_var_default_params(pt_spatial_var_params* out);
/* The statement on the host: moments W*H*2 floats, length and variance W*H,
 * guide W*H*4, out W*H, distinct from every input.  Pure host function. */
int pt_spatial_variance_host(const float* moments, const float* length, const float* variance, const float* guide,
                             int width, int height, const pt_spatial_var_params* params, float* out);
/* Enqueues the statement on the context's stream; all pointers are device
 * memory, moments 8-B aligned, length and variance 4-B, the guide 16-B, out
 * 4-B and distinct from every input (PT_ERR_INVALID).  The same bits as the
 * host function. */
int pt_spatial_variance(pt_context* ctx, const void* moments, const void* length, const void* variance,
                        const void* guide, int width, int height, const pt_spatial_var_params* params, void* out);
/* pt_temporal_denoise with pass 0's variance plane replaced by the estimate
 * from the temporal result's moments, length, variance and guide, written to a
 * library-owned plane: the temporal result (pt_temporal_device_ptr 0-3) is
 * only read, so the history is not disturbed.  filter_params and
 * spatial_params null: the defaults of each; dst_device as for
 * pt_temporal_denoise.  Errors: those of pt_temporal_denoise, and bad
 * spatial_params.  When no pixel is short it gives pt_temporal_denoise's bits. */
int pt_temporal_denoise_spatial(pt_context* ctx, const pt_denoise_var_params* filter_params,
                                const pt_spatial_var_params* spatial_params, void* dst_device);

/* ---- adaptive sampling: stop converged tiles, keep sampling the others ---
 * pt_render gives every pixel the same number of samples.  The calls below
 * feed the variance of the mean back into the sampler: each 16x16 tile of the
 * frame (the partition unit; tiles are numbered in raster order here, b =
 * by * blocks_x + bx, not in the partition's rotated order) carries its own
 * sample count n_T, and a tile stops once every pixel of it is converged.
 *
 * The contract: seeds go by pixel and batch, so after an adaptive render every
 * pixel of tile T inside the frame holds, in the accumulation image and in the
 * moments image, exactly the bits pt_render(0, n_T) would leave there under
 * the same options and seed base (PT_OPT_MOMENTS 1).
 *
 * The rule, shared by the kernel and the host function (every operation rounds
 * once, the division and the square root are IEEE, nothing is fused; fmax is
 * maxNum).  For a tile with count n and each pixel p of it inside the frame,
 * from the moments {m1, m2}:
 *   finite_p = fabs(m1_p) <= FLT_MAX && fabs(m2_p) <= FLT_MAX
 *   e_p  = finite_p ? sqrt(fmax(0, m2_p - m1_p * m1_p) / float(n - 1)) / fmax(m1_p, lum_floor) : +inf
 *   pixel converged:  e_p <= threshold
 *   tile converged:   every pixel of it inside the frame converged
 *   E_T  = fmax over those pixels of e_p, from +0      (reported; the decision is the predicate)
 *   next = n                            if converged or n >= max_batches
 *          min(n + step, max_batches)   otherwise
 * maxNum would drop a NaN moment (the clamp makes its variance 0); finite_p
 * keeps a pixel with a NaN or infinite moment from ever counting as converged:
 * its tile stops at max_batches only.  For finite moments e_p is finite and
 * >= +0, so neither the predicate nor the maximum depends on the order of the
 * reduction.  A fully culled tile has zero moments, e_p = 0, and stops at
 * min_batches.  n >= 2 (n - 1 divides).
 *
 * Parameters: 2 <= min_batches <= max_batches <= 65536, step >= 1, threshold
 * and lum_floor finite and > 0; null: the defaults.  Anything else:
 * PT_ERR_INVALID.  Defaults (pt_adaptive_default_params): min 4, max 64, step
 * 15 (four rounds), threshold 0.09, lum_floor 2: the floor that gave the lowest
 * error at equal samples on the box at 1080p, and the threshold that spent 16
 * samples per pixel there.  lum_floor is in the scene's luminance units (the
 * reference light's intensity is 10): below it the rule bounds the absolute
 * standard error of the mean at threshold * lum_floor, above it the relative
 * one. */
typedef struct pt_adaptive_params {
  uint32_t min_batches, max_batches, step;
  float threshold, lum_floor;
} pt_adaptive_params;
int pt_adaptive_default_params(pt_adaptive_params* out);
/* The rule on the host: moments W*H*2 floats, counts one per tile (raster
 * order, each >= 2), next_counts and errors (E_T) one per tile; errors may be
 * null.  Pure host function. */
int pt_adaptive_select_host(const float* moments, const uint32_t* counts, int width, int height,
                            const pt_adaptive_params* params, uint32_t* next_counts, float* errors);
/* Enqueues the rule on the context's stream over the caller's device images:
 * moments 8-B aligned, counts, next_counts and errors 4-B; next_counts may be
 * counts.  The same bits as the host function. */
int pt_adaptive_select(pt_context* ctx, const void* moments, const void* counts, int width, int height,
                       const pt_adaptive_params* params, void* next_counts, void* errors);
/* Starts an adaptive render: clears the accumulator and the moments, sets every
 * count to 0 and enqueues round 0, in which every tile renders batches
 * 0..min_batches-1 (at the seed base PT_OPT_SEED_BASE).  PT_ERR_INVALID without
 * PT_OPT_MOMENTS 1, a scene, lights, a camera or a frame; PT_ERR_UNSUPPORTED on
 * multi-device contexts, a partition of more than one rank, in stats mode, with
 * PT_OPT_COUNT_TRACED and, unless PT_OPT_ADAPTIVE_WF is 1, with PT_OPT_KERNEL 3
 * (under auto the adaptive calls then run the path-recursive kernel). */
int pt_adaptive_begin(pt_context* ctx, const pt_adaptive_params* params);
/* Enqueues up to `rounds` rounds: the rule over all tiles, the list of the
 * tiles whose count grew (ascending), and one launch that renders each listed
 * tile's new batches.  Nothing is waited for: the launch is sized for every
 * tile and reads the list's length from device memory.  After
 * ceil((max_batches - min_batches) / step) rounds no count can change, and
 * further rounds are no-ops.  PT_ERR_INVALID without pt_adaptive_begin. */
int pt_adaptive_advance(pt_context* ctx, uint32_t rounds);
/* Waits for the rounds enqueued so far.  rounds_done: rounds enqueued since
 * pt_adaptive_begin (round 0 not counted); live_tiles: tiles the last round
 * rendered (after pt_adaptive_begin alone: every tile), 0 once no round is
 * left; samples_total: the sum over tiles of n_T times the tile's pixels
 * inside the frame.  Each pointer may be null. */
int pt_adaptive_info(pt_context* ctx, uint32_t* rounds_done, uint32_t* live_tiles, unsigned long long* samples_total);
/* Waits and copies the tiles' counts n_T and the errors E_T of the last round's
 * rule (0 before the first round); n_tiles must be the frame's tile count;
 * either pointer may be null. */
int pt_adaptive_read_counts(pt_context* ctx, uint32_t* counts, float* errors, size_t n_tiles);
/* Waits and copies the last round's live list: up to max_entries entries of
 * four ints {x0, y0, first_batch, n_batches}, their number in *n_live. */
int pt_adaptive_read_live(pt_context* ctx, int* entries, size_t max_entries, uint32_t* n_live);
/* Device memory of the adaptive state: which = 0 counts (uint32 per tile), 1
 * errors (float per tile), 2 the variance plane pt_adaptive_denoise wrote (W*H
 * floats); null when there is none. */
void* pt_adaptive_device_ptr(pt_context* ctx, int which);
/* pt_denoise_var's passes on the adaptive result: a kernel writes the variance
 * plane var_p = fmax(0, m2_p - m1_p * m1_p) / float(n_T - 1) at each tile's own
 * count, and the variance-plane passes run on it with the guide (rendered if
 * there is none); the same bits as pt_denoise_var_plane_host fed with that
 * plane.  dst_device as for pt_denoise_var.  PT_ERR_INVALID without an adaptive
 * render.
 *
 * After an adaptive render pt_read_accum works as ever; the moments have no
 * single n, so pt_read_moments reports n = 0 and pt_denoise_var refuses, as
 * after a render with a gap.  The adaptive state ends with pt_upload_scene,
 * pt_scene_upload, pt_upload_lights, pt_set_params, a change of frame size or
 * of the bound buffer, pt_clear_accum and any render (pt_render, pt_dispatch,
 * pt_render_packed, pt_temporal_advance). */
int pt_adaptive_denoise(pt_context* ctx, const pt_denoise_var_params* params, void* dst_device);

/* ---- display transform: exposure, tone map, 8-bit sRGB out ---------------
 * The last step of the reference's loop on the device: a W x H float4 image
 * becomes one packed RGBA8 word a pixel (r the lowest byte, alpha 255), in the
 * row order of the source, so a display or an encoder reads a quarter of the
 * bytes.  The statement (csrc/pt_display.h), per pixel, alpha not read:
 *
 *   v = c * scale              scale = exposure, or exposure * auto_scale
 *   v = min(max(v, 0), 2^40)   IEEE minNum/maxNum: NaN -> 0, -x -> 0, +inf -> 2^40
 *   PT_TONEMAP_CLAMP     nothing: an sRGB swapchain showing the float image
 *   PT_TONEMAP_REINHARD  L = lum(v); Lp = (L * (1 + L / (white * white))) / (1 + L);
 *                        v = v * (Lp / L) when L > 0
 *   PT_TONEMAP_ACES      (x * (2.51 x + 0.03)) / (x * (2.43 x + 0.59) + 0.14) per channel
 *   code = the 8-bit sRGB code of v: exactly what PT_IMAGE_PNG encodes, for
 *          every float (a table of 255 thresholds, checked against the
 *          double-precision statement for all 2^32 bit patterns)
 *
 * With the default parameters the bytes are those pt_write_image puts into a
 * PNG.  Every operation is a single IEEE fp32 operation in the stated order, so
 * pt_display and pt_display_host give the same bytes.
 *
 * auto_exposure 1 meters the source first: the pixels whose luminance
 * L = lum(max(c, 0)) is finite and > 0 (a culled background of exact zeros does
 * not count), the sum of log(L) over them by a fixed tree (per 16x16 tile, then
 * over the tiles; pt_display.h), mean = sum / n, target = key / exp(mean).  The
 * first metering call after a reset uses auto_scale = target, a later one
 * prev + (target - prev) * adapt (adapt 1: target), prev being the scale the
 * call before used; a source with no metered pixel keeps prev, or 1 without
 * one.  The scale lives in device memory and the display kernel reads it from
 * there: nothing waits on the host.  It survives across calls (eye adaptation
 * in a pt_temporal_advance loop); pt_display_reset, a change of frame size or
 * of the bound buffer and a scene upload forget it. */
#define PT_TONEMAP_CLAMP 0
#define PT_TONEMAP_REINHARD 1
#define PT_TONEMAP_ACES 2
typedef struct pt_display_params {
  int   tonemap;        /* PT_TONEMAP_CLAMP | _REINHARD | _ACES */
  float exposure;       /* finite, > 0; default 1 */
  int   auto_exposure;  /* 0 | 1; default 0 */
  float key;            /* finite, > 0; default 0.18 */
  float white;          /* finite, > 0, white*white finite non-zero; default 4 */
  float adapt;          /* in (0, 1]; default 1 */
} pt_display_params;
int pt_display_default_params(pt_display_params* out);
/* Enqueues the transform of src_device (null: the accumulation image; else any
 * W x H float4 image of the context's frame size, 16-B aligned: pt_denoise's,
 * pt_temporal_device_ptr's, ...) into dst_device (null: a library-owned image,
 * pt_display_device_ptr / pt_read_display; else W*H 32-bit words, 4-B aligned,
 * not overlapping the source).  params null: the defaults.  PT_ERR_INVALID for
 * bad parameters or without an accumulation image (it gives the frame size);
 * PT_ERR_UNSUPPORTED on a pt_create_multi context, as every call below that
 * takes a context. */
int pt_display(pt_context* ctx, const pt_display_params* params, const void* src_device, void* dst_device);
/* The library-owned image of the last pt_display with a null destination; null
 * when there is none of the current frame size. */
void* pt_display_device_ptr(pt_context* ctx);
/* Waits and copies that image: n_bytes >= W*H*4. */
int pt_read_display(pt_context* ctx, unsigned char* rgba8, size_t n_bytes);
/* Waits.  auto_scale: the scale the last metering pt_display used (1 when none
 * has run since the state was forgotten); n_metered: the pixels it metered.
 * Either pointer may be null. */
int pt_display_exposure(pt_context* ctx, float* auto_scale, uint32_t* n_metered);
int pt_display_reset(pt_context* ctx);
/* The 8-bit sibling of pt_readback_begin/end: the display kernel writes the
 * snapshot itself (4 B a pixel instead of a 16-B device-to-device copy), and
 * the copy to pinned host memory on the second stream moves W*H*4 bytes.  Two
 * slots and the same ticket rules: a third begin recycles the older slot, whose
 * ticket is then unknown; a ticket is collected once. */
int pt_display_readback_begin(pt_context* ctx, const pt_display_params* params, const void* src_device, int* ticket);
int pt_display_readback_end(pt_context* ctx, int ticket, unsigned char* rgba8, size_t n_bytes);
/* The same transform on the host, of a W x H RGBA32F image into W*H*4 bytes.
 * auto_scale_io (metering only; may be null): in, the previous scale or 0 for
 * none; out, the scale this call used. */
int pt_display_host(const float* rgba, int w, int h, const pt_display_params* params,
                    float* auto_scale_io, unsigned char* rgba8);

/* ---- guide-driven upsampling: render at 1/s size, present at full size ----
 * An interactive host lowers the render size while the camera moves and still
 * presents a full-size frame.  The context stays at the render size w x h; the
 * calls below put a w x h float4 image onto the W x H = (s*w) x (s*h) grid by
 * joint bilateral upsampling (Kopf et al. 2007) under the full-size guide image
 * {n.xyz, t}, which costs one ray a pixel and carries the silhouettes.
 *
 * A pixel's samples are jittered around ndc = 2 * px / W - 1, the pixel's
 * lattice point, so pixel (i, j) of the w x h frame looks along exactly the
 * guide ray of pixel (s*i, s*j) of the full frame (pt_guide_ray gives the same
 * bits for both): the rendered frame is the full frame sampled at every s-th
 * lattice point, its guide is the full guide at stride s, and one guide serves
 * both ends of a tap.  The statement (csrc/pt_upsample.h), for the output pixel
 * (X, Y), src the w x h image and G the full guide:
 *
 *   i0 = X / s, j0 = Y / s;  fx = float(X - i0*s) / float(s), fy likewise
 *   bx = {1 - fx, fx}, by = {1 - fy, fy}
 *   over the taps (i0 + di, j0 + dj), dj = 0..1 outer, di = 0..1 inner, those
 *   outside the w x h frame and those with bx[di] == 0 or by[dj] == 0 skipped:
 *     gq = G[(j*s) * W + i*s], gp = G[Y * W + X]
 *     d2n = (nx*nx + ny*ny) + nz*nz over gp.xyz - gq.xyz;  dz = gp.w - gq.w
 *     wt  = (bx[di] * by[dj]) * exp(-(d2n / sn2 + (dz*dz) / sz2))
 *     sum.rgb += wt * src[j*w + i].rgb;  sum.w += wt
 *   out.rgb = sum.w > 0 ? sum.rgb / sum.w : src[j0*w + i0].rgb;  out.a = src[j0*w + i0].a
 *
 * sn2 = sigma_normal^2, sz2 = sigma_depth^2.  Every operation is a single IEEE
 * fp32 operation in the stated order and exp the library's own, so the device
 * calls and pt_upsample_host give the same bits.  At the lattice points the
 * result is the rendered value (out[s*j][s*i] == src[j][i]; a -0 comes out +0):
 * one tap is left, its guide is the pixel's own, its weight exactly 1.  A hit
 * beside a miss weighs 0 (dz * dz = inf), so silhouettes stay where the full
 * guide has them; a tap of zero bilinear weight is skipped, so a NaN or
 * infinite colour reaches only the pixels strictly inside its four cells.  The
 * fallback src[j0*w + i0] applies when no tap is left a weight (also when a NaN
 * guide makes the sum NaN).
 *
 * Time and error against a full-size render: profiles/upsample/, DESIGN.md
 * section 9h. */
typedef struct pt_upsample_params {
  int   scale;          /* s: 2 to 8; default 2 */
  float sigma_normal;   /* finite, > 0, its square finite and non-zero; default 0.35 */
  float sigma_depth;    /* the same; default 0.25 */
} pt_upsample_params;
int pt_upsample_default_params(pt_upsample_params* out);
/* The statement on the host: src w*h*4 floats, guide_full (s*w)*(s*h)*4 floats,
 * out as many.  PT_ERR_INVALID for bad parameters, and for a full frame of more
 * than 2^31 pixels; a 1x1 source is valid.  params null: the defaults. */
int pt_upsample_host(const float* src, int w, int h, const float* guide_full, const pt_upsample_params* params,
                     float* out);
/* Enqueues the statement on explicit device images, as pt_reproject and
 * pt_spatial_variance take theirs: src_device w x h float4, guide_full_device
 * and dst_device (s*w) x (s*h) float4, all 16-B aligned, the destination
 * overlapping neither input.  dst_device null: a library-owned image
 * (pt_upsampled_device_ptr, pt_read_upsampled).  Needs no scene, camera or
 * frame.  PT_ERR_UNSUPPORTED on a pt_create_multi context, as every call below
 * that takes a context. */
int pt_upsample_images(pt_context* ctx, const pt_upsample_params* params, const void* src_device, int w, int h,
                       const void* guide_full_device, void* dst_device);
/* The same with the context's own inputs.  The context stays at the render
 * size w x h (pt_resize_and_clear / pt_bind_accum).  src_device null: the
 * accumulation image; else any w x h float4 image (pt_denoise's,
 * pt_temporal_device_ptr's, the adaptive filter's).  dst_device null: the
 * library-owned (s*w) x (s*h) image.  The call renders the full-size guide
 * itself into a library-owned image (pt_upsample_guide_device_ptr), by the
 * launch pt_render_guide makes, with the frame size (s*w) x (s*h) and the walk
 * that pt_render_guide would take, and keeps it until the scene, the camera,
 * the frame size or the scale changes: while none does, a call launches the
 * upsampling kernel alone.  The context's own w x h guide (pt_render_guide) is
 * neither read nor written.  PT_ERR_INVALID without a scene, a camera or a
 * frame. */
int pt_upsample(pt_context* ctx, const pt_upsample_params* params, const void* src_device, void* dst_device);
/* The library-owned image of the last pt_upsample or pt_upsample_images with a
 * null destination (null: none), and its copy to the host behind the enqueued
 * work: n_floats >= W*H*4 of that image (pt_upsample_info gives W and H). */
void* pt_upsampled_device_ptr(pt_context* ctx);
int pt_read_upsampled(pt_context* ctx, float* rgba, size_t n_floats);
/* The full-size guide pt_upsample keeps, (s*w) x (s*h) float4; null when there
 * is none for the current scene, camera and frame size. */
void* pt_upsample_guide_device_ptr(pt_context* ctx);
/* info[0] the scale of the kept guide (0: none for the current inputs), [1] and
 * [2] its width and height, [3] the guide launches pt_upsample and
 * pt_upsample_display have made on this context (a call that finds its guide
 * kept adds none), [4] and [5] the size of the library-owned upsampled image,
 * [6] and [7] that of the library-owned upsampled display image (0: none). */
int pt_upsample_info(pt_context* ctx, int info[8]);
/* pt_upsample and pt_display in one kernel: the upsampled pixel goes through
 * the display transform (display_params; null: the defaults) and is written as
 * the RGBA8 word; the full-size float image is never written or read back,
 * 32 B a pixel less.  The bytes are those of pt_display_host of
 * pt_upsample_host's image.  With auto_exposure the metering sees the rendered
 * w x h pixels (src_device), not the upsampled ones: it is the metering launch
 * and state of pt_display, so the scale adapts across pt_display and this call
 * alike, and pt_display_exposure / pt_display_reset apply.  dst_device null: a
 * library-owned image (pt_display_upsampled_device_ptr,
 * pt_read_display_upsampled: n_bytes >= W*H*4); else W*H 32-bit words, 4-B
 * aligned. */
int pt_upsample_display(pt_context* ctx, const pt_upsample_params* upsample_params,
                        const pt_display_params* display_params, const void* src_device, void* dst_device);
void* pt_display_upsampled_device_ptr(pt_context* ctx);
int pt_read_display_upsampled(pt_context* ctx, unsigned char* rgba8, size_t n_bytes);

/* ---- batched ray queries: closest hit and occlusion -------------------- */
/* The caller's own rays against the uploaded scene, answered by the walks the
 * renderer uses, bit for bit the reference's traceRay (raytrace_comp.comp
 * :159-204) and occluded() statement (:359, :398).  Needs a scene and nothing
 * else: no camera, lights or frame.
 *
 * PT_RAYS_CLOSEST writes a pt_hit per ray: the accepted triangle of least t of
 * the exhaustive walk, ties to the first visited.  tri is the leaf's triangle
 * index as the shader reads it: triangle indices[3*tri .. 3*tri+2] of the
 * arrays given to pt_upload_scene.  n is normalize(cross(e1, e2)) of that
 * triangle, u and v intersectTriangle's own barycentrics (the point is
 * (1-u-v) v0 + u v1 + v v2).  A miss is {1e30f, -1, 0, 0, {0, 0, 0}, 0}.  limit
 * and reserved of the ray are ignored; reserved of a hit is written 0.
 * PT_RAYS_ANY writes a uint32_t per ray: 1 iff some triangle the reference
 * would test is accepted with t < 1e30f && !(t >= limit), else 0.  A NaN
 * limit therefore makes any accepted hit occlude.
 *
 * Directions are taken as given, t is in units of |d|, and no ray is refused:
 * zero, NaN, infinite and subnormal components get the exact walk's answer.
 * Normalise directions all the same: a scene with a wide tree (pt_wide_info,
 * PT_OPT_WIDE not 0) is walked by the culled wide walk only for rays with
 * dot(d, d) <= 1.00002, a finite 1/d on every axis and |o| <= 1e15; any other
 * ray takes the exact threaded walk, which is correct and, on a big scene,
 * slow.  PT_OPT_SCENE_IN_LDS, PT_OPT_WIDE, PT_OPT_WIDE_NODE, PT_OPT_WF_GRID,
 * PT_OPT_WF_REFILL and PT_OPT_RAYS_REFILL choose the walk; the answers are the
 * same bits under all of them.  Queries are not counted by stats mode
 * (pt_get_stats) or PT_OPT_COUNT_TRACED (pt_get_traced).
 *
 * PT_ERR_INVALID: no scene, a null pointer with n > 0, an unknown kind, a
 * device pointer not 16-B aligned, n > 2^31 - 256.  PT_ERR_UNSUPPORTED on a
 * pt_create_multi context.  n == 0 is a successful no-op. */
typedef struct pt_ray { float o[3]; float d[3]; float limit; uint32_t reserved; } pt_ray;          /* 32 B */
typedef struct pt_hit { float t; int32_t tri; float u, v; float n[3]; uint32_t reserved; } pt_hit;  /* 32 B */
#define PT_RAYS_CLOSEST 0   /* out: n pt_hit */
#define PT_RAYS_ANY 1       /* out: n uint32_t, 1 = occluded, 0 = not */
/* d_rays: n pt_ray, d_out: n answers, both device memory, distinct.  Enqueued
 * on the context's stream; waits for nothing. */
int pt_trace_rays(pt_context* ctx, int kind, const void* d_rays, size_t n, void* d_out);
/* The same from and to host memory, staged through library-owned buffers;
 * returns when the answers are in `out`. */
int pt_trace_rays_sync(pt_context* ctx, int kind, const pt_ray* rays, size_t n, void* out);
/* The host statement of both kinds, without a context or a GPU: the
 * reference's depth-first walk over the vertex, index and node arrays of
 * pt_upload_scene (flags: PT_NODES_INT_BITS), `threads` host threads (<= 0:
 * one per core).  PT_ERR_SCENE for arrays pt_upload_scene would refuse. */
int pt_trace_rays_host(const float* vertices, size_t n_vertex_floats, const uint32_t* indices, size_t n_indices,
                       const pt_bvh_node* nodes, size_t n_nodes, uint32_t flags, int kind, const pt_ray* rays,
                       size_t n, void* out, int threads);

/* ---- radiance queries: path-trace the caller's own rays ---------------- */
/* What radiance arrives along a given ray: the shader's pathTrace
 * (raytrace_comp.comp:300-418) from the caller's origin, direction and seed,
 * with the lights of pt_upload_lights and max_depth / sss_bounces of
 * pt_set_params, bit for bit what pt_render computes for a pixel whose ray and
 * seed these are.  Needs a scene and parameters; zero lights are valid; no
 * camera and no frame.
 *
 * A query is a pt_ray read as {o, d, -, seed}: limit is ignored and reserved
 * is the path's seed, so rays made for pt_trace_rays are queries with seed 0.
 * Sample s = 0 .. n_samples-1 of a query is
 *   c_s = pathTrace(o, d, seed + s * seed_stride)        (uint32 wrap-around)
 * -- the re-seed rng = seed (:307), the light pre-pass on the given ray
 * (:311-328), then the bounces -- and the answer is the shader's running mean
 * (:467-469) of them in order from {+0, +0, +0, +0}:
 *   acc.rgb = (acc.rgb * float(s) + c_s) / float(s + 1)
 *   acc.a   = (acc.a   * float(s) + 1)   / float(s + 1)
 * always applied, so one sample is (0 * 0 + c) / 1 and a -0 radiance comes
 * out +0.  d is taken as given and never normalised; no ray is refused:
 * pt_trace_radiance_host defines the answer for NaN, infinite, zero and
 * subnormal components and the device equals it (NaN where NaN, every other
 * float the same bits).
 *
 * Nothing that belongs to a camera applies: not PT_OPT_SEED_BASE, not the
 * primary culling.  Queries are not counted by stats mode (pt_get_stats) or
 * PT_OPT_COUNT_TRACED (pt_get_traced) and leave the accumulation image
 * untouched.  The kernel family, the LDS staging, the sweep and wide walks and
 * the exit skip are chosen by pt_render's own rules for a launch of as many
 * paths (PT_OPT_KERNEL, PT_OPT_SCENE_IN_LDS, PT_OPT_SMALL_SWEEP, PT_OPT_WIDE,
 * PT_OPT_WIDE_NODE, PT_OPT_WF_GRID, PT_OPT_EXIT_SKIP, ...); the answers are the
 * same bits under all of them.  Work is cut into chunks of whole queries
 * (PT_OPT_RADIANCE_CHUNK); the path buffers are the library's, allocated on
 * demand and freed with the context.
 *
 * PT_ERR_INVALID: no scene, a null pointer with n > 0, n_samples outside
 * 1 .. 65536, a device pointer not 16-B aligned, d_out overlapping d_rays,
 * n > 2^31 - 256.  PT_ERR_UNSUPPORTED on a pt_create_multi context, and where
 * PT_OPT_SCENE_IN_LDS 2 asks for a staging the scene does not fit.  n == 0 is
 * a successful no-op. */
typedef struct pt_radiance_params {
  uint32_t n_samples;    /* samples folded into each answer, 1 .. 65536 */
  uint32_t seed_stride;  /* sample s draws from seed + s * seed_stride */
} pt_radiance_params;
/* {1, 1}: one sample; with more, consecutive seeds. */
int pt_radiance_default_params(pt_radiance_params* out);
/* d_rays: n pt_ray, d_out: n float4 {r, g, b, a}, both device memory, distinct.
 * params null: the defaults.  Enqueued on the context's stream; waits for
 * nothing. */
int pt_trace_radiance(pt_context* ctx, const pt_radiance_params* params, const void* d_rays, size_t n, void* d_out);
/* The same from and to host memory (out: 4 n floats), staged in chunks through
 * library-owned buffers; returns when the answers are in `out`. */
int pt_trace_radiance_sync(pt_context* ctx, const pt_radiance_params* params, const pt_ray* rays, size_t n,
                           float* out);
/* The host statement, without a context or a GPU: pathTrace in pt_math.h's
 * IEEE forms over the vertex, index and node arrays of pt_upload_scene (flags:
 * PT_NODES_INT_BITS), every ray the reference's depth-first walk, the lights'
 * frames as pt_upload_lights derives them; `threads` host threads over the
 * queries (<= 0: one per core), the same bytes whatever their number.
 * PT_ERR_SCENE for arrays pt_upload_scene would refuse; PT_ERR_INVALID for
 * negative max_depth or sss_bounces. */
int pt_trace_radiance_host(const float* vertices, size_t n_vertex_floats, const uint32_t* indices, size_t n_indices,
                           const pt_bvh_node* nodes, size_t n_nodes, uint32_t flags, const pt_area_light* lights,
                           size_t n_lights, int max_depth, int sss_bounces, const pt_radiance_params* params,
                           const pt_ray* rays, size_t n, float* out, int threads);
/* main()'s own ray (:430-460) of a pixel and a sample batch, as a query: the
 * aperture draw, the jitter draw and the focal point of the context's camera
 * and frame size, from the seed (batch * H + y) * W + x, which is also written
 * to reserved; limit is written 1e30f.  pt_trace_radiance of these rays is the
 * colour pt_render folds for that pixel and batch; a caller building another
 * camera model starts from them.  d_pixels: n int32 y * W + x in device memory,
 * each inside the frame, or null = every pixel in raster order (then
 * n <= W * H); d_rays: n pt_ray, device memory, 16-B aligned.  Needs a camera
 * and a frame size (pt_resize_and_clear / pt_bind_accum), no scene.  Enqueued
 * on the context's stream. */
int pt_camera_rays(pt_context* ctx, uint32_t batch, const int32_t* d_pixels, size_t n, void* d_rays);
/* The host statement: camera_ubo as pt_set_camera takes it, pixels in host
 * memory (checked: PT_ERR_INVALID for one outside the frame). */
int pt_camera_rays_host(const float camera_ubo[16], int width, int height, uint32_t batch, const int32_t* pixels,
                        size_t n, pt_ray* rays);

/* ---- multi-GPU screen-space partition ------------------ */
/* Pixels are grouped into 16x16 blocks.  Block (bx, by) is tile
 * b = by*blocks_x + (bx - by) mod blocks_x (rows rotated by their index, so
 * ranks get anti-diagonal stripes, not column stripes); this context renders
 * tile b iff b % nranks == rank.  pt_clear_accum then writes +0 to
 * owned pixels and -0 (the IEEE additive identity) to the others, so a sum
 * reduction of all ranks' buffers is bit-identical to a single-GPU frame. */
int pt_set_partition(pt_context* ctx, int nranks, int rank);
/* Unequal shares: tiles are dealt in periods of sum(slots) slots, rank r
 * owning slots[r] consecutive ones (1..64 each, at most 4096 in all).
 * pt_set_partition is the case of one slot per rank.  Every rank must pass
 * the same slots.  bench.py gives the root, which also assembles the
 * gathered frame, fewer slots. */
int pt_set_partition_slots(pt_context* ctx, int nranks, int rank, const int* slots);
/* Gather-based assembly (cheaper than a full-frame sum for N > 2): a rank
 * packs the tiles it owns into a dense device buffer of
 * n_tiles * 16*16 float4 (pt_tiles_owned), ships it to the root, and the
 * root unpacks each rank's buffer into a W x H frame.  The frame size and
 * partition are the context's; all work is enqueued on its stream. */
int pt_tiles_owned(pt_context* ctx, int* n_tiles);
int pt_tiles_pack(pt_context* ctx, void* dst_device);
int pt_tiles_unpack(pt_context* ctx, const void* src_device, int src_rank, void* frame_device);
/* Sparse exchange of the last rendered frame: only the tile parts ("items",
 * 256/SPL pixels each) that can hold a live pixel under primary culling.
 * Every rank must have rendered the same frame (camera, size, partition
 * size, batches).  pt_items_live: rank's live item count and pixels per item
 * (a slot must hold n_items*item_pixels float4).  pt_items_pack: this rank's
 * live items, densely.  pt_items_unpack_all: rank r's slot at
 * src + r*slot_floats; live items are scattered into the frame, culled ones
 * written as (0,0,0,1) — their value for a frame rendered from batch 0, which
 * this call requires.  With culling off every item is live. */
int pt_items_live(pt_context* ctx, int rank, int* n_items, int* item_pixels);
int pt_items_pack(pt_context* ctx, void* dst_device);
int pt_items_unpack_all(pt_context* ctx, const void* src_device, size_t slot_floats, void* frame_device);
/* pt_render_packed: render a fresh frame (batches 0..n_batches-1, as
 * pt_clear_accum + pt_render) and write this rank's live items straight into
 * dst_device in the pt_items_pack layout — what pt_render + pt_items_pack
 * give, in one launch, without the culled-item fill.  The accumulation buffer
 * is neither read nor written.  gathered_device (optional, else null): the
 * per-rank slots of the PREVIOUS frame, which the same launch assembles into
 * frame_device exactly as pt_items_unpack_all would — the root's step of a
 * pipelined tile split is then one launch; that frame must have been
 * rendered by pt_render_packed with the same item layout — frame size,
 * partition, sample lanes, culling rectangles, item order (error otherwise).
 * Replaces, for the tile split, the reference's one dispatch per frame plus
 * image readback (VulkanRayTracer.cpp:803-865). */
int pt_render_packed(pt_context* ctx, uint32_t n_batches, void* dst_device, const void* gathered_device,
                     size_t slot_floats, void* frame_device);
/* The item tables behind pt_items_live / pt_items_pack / pt_items_unpack_all
 * and pt_render_packed, as a pure host function (no context, no GPU): rank's
 * live items (tile parts that can hold a live pixel) in launch order, its
 * culled items, and -- when pixel_of is not null -- for every listed item
 * (live first, then culled) and each of its 256/sample_lanes slots q the
 * pixel index y*W+x it carries, or -1 past the frame edge.  slots: null for
 * one slot per rank, else as pt_set_partition_slots.  cull_rects / n_cull: as
 * pt_primary_cull_rects returns them (n_cull < 0: no culling, every item is
 * live).  item_order: PT_OPT_ITEM_ORDER.  Call with null live/culled to get
 * the counts; *n_live / *n_culled give the buffer sizes on input. */
int pt_partition_items(int width, int height, int sample_lanes, int nranks, int rank, const int* slots,
                       const float* cull_rects, int n_cull, int item_order, int* live, size_t* n_live,
                       int* culled, size_t* n_culled, int* pixel_of);

/* ---- native multi-GPU step loop (RCCL) ------------------ */
/* The tile split's pipelined sparse gather with the collective issued from
 * C++: frames alternate between two internal streams; frame k's launch
 * renders this rank's live items into a send slot and, on the root, assembles
 * frame k-2 (pt_render_packed); a grouped RCCL send/recv on a high-priority
 * stream gathers every rank's slot on rank 0.  RCCL (librccl.so.1) is loaded
 * at run time -- the copy already in the process if there is one -- so the
 * single-GPU library needs none.
 * pt_dist_unique_id: rank 0 makes the communicator id (128 bytes), which the
 * caller broadcasts (e.g. over torch.distributed); pt_dist_init: every rank,
 * collectively, after setting the same partition (or, to time the root's
 * step on one GPU, nranks = 1 with an N-way partition on rank 0: the other
 * ranks' slots then arrive as a device copy of the same bytes -- an
 * emulation, not a gather); pt_dist_run: n_frames frames of n_batches
 * samples (batch 0..n-1, fresh) on 1 to 3 alternating streams (2 or 3: a
 * frame's tail overlaps the next ones' heads; max(2, n_streams) frames are
 * in flight before the root assembles one); the root writes frame j
 * to frames + (j % n_frame_bufs) * W*H*4 floats (device memory; ignored on
 * other ranks).  Every rank must have rendered the frame's configuration once
 * with pt_render (it fixes the item layout).  Work is enqueued; the frames
 * are complete after pt_synchronize.  pt_dist_finalize frees it (also done
 * by pt_destroy).  Replaces, for the tile split, the reference's
 * dispatch-and-readback per frame (VulkanRayTracer.cpp:803-865). */
#define PT_DIST_ID_BYTES 128
int pt_dist_unique_id(void* id, size_t id_bytes);
int pt_dist_init(pt_context* ctx, const void* id, int nranks, int rank);
int pt_dist_run(pt_context* ctx, uint32_t n_batches, int n_frames, int n_streams, void* frames_device,
                int n_frame_bufs);
/* Run the loop on caller-owned streams (e.g. torch streams) instead of the
 * ones it creates: the first two render streams and the gather stream (null
 * keeps the library's own).  With caller render streams pt_dist_run takes at
 * most 2 streams (PT_ERR_INVALID for 3, which would mix in a library stream
 * outside the caller's ordering).  The library creates its render streams at the least priority
 * and the gather stream at the greatest: the HIP runtime keeps a pool of
 * GPU_MAX_HW_QUEUES hardware queues per priority, so each render stream gets
 * a queue of its own. */
int pt_dist_set_streams(pt_context* ctx, void* render_stream0, void* render_stream1, void* gather_stream);
int pt_dist_slot_floats(pt_context* ctx, size_t* slot_floats);
/* Wait (polling) up to timeout_ms for the loop's streams; PT_ERR_HIP on
 * timeout.  pt_dist_abort: ncclCommAbort + free, after such a timeout. */
int pt_dist_wait(pt_context* ctx, int timeout_ms);
int pt_dist_abort(pt_context* ctx);
/* The communicator's rank count as RCCL reports it (ncclCommCount; -1 if
 * the loaded library lacks it), and the rank count / rank pt_dist_init took. */
int pt_dist_info(pt_context* ctx, int* comm_ranks, int* nranks, int* rank);
int pt_dist_finalize(pt_context* ctx);

/* ---- kernel options ---------------------------------------------------- */
/* PT_OPT_SCENE_IN_LDS: stage the scene in LDS per workgroup — 0 never,
 * 1 when it fits in 48 KB (default), 2 always (error if it does not fit).
 * Output is identical either way. */
#define PT_OPT_SCENE_IN_LDS 1
/* PT_OPT_SAMPLE_LANES: lanes that trace one pixel's samples side by side in
 * pt_render — 0 auto (scenes in device memory 8; LDS-resident scenes 4 on a
 * whole frame or a partition of 8 or more ranks, 2 on 2-7 ranks; never more
 * lanes than samples), or 1, 2, 4, 8.  Output is identical for every value. */
#define PT_OPT_SAMPLE_LANES 2
/* PT_OPT_FRESH_BATCH0: 1 = a launch whose first batch is 0 starts from a
 * cleared (+0) accumulator without reading it — bitwise what
 * pt_clear_accum + pt_render give, minus a clear and a read of the image.
 * 0 (default) = read the accumulator, as the reference does (prev * 0). */
#define PT_OPT_FRESH_BATCH0 3
/* PT_OPT_KERNEL: 0 auto (wavefront for scenes of >= 32768 triangles that
 * are not LDS-resident, else path-recursive), 1 path-recursive, 3 wavefront
 * pipeline (paths held in device memory, traversal and shading in separate
 * kernels; 416 bytes of device memory per pixel x sample, at most 2^27 paths
 * per chunk; not with stats mode; auto picks it from 16384 triangles with the
 * culled wide walk).  Output is identical for every value.  2 (a lane state
 * machine, measured slower on every scene) was removed: PT_ERR_UNSUPPORTED,
 * as is PT_OPT_SM_BATCH, its only knob. */
#define PT_OPT_KERNEL 4
#define PT_OPT_SM_BATCH 5
/* PT_OPT_PRIMARY_CULL: 1 (default) = a pixel whose every possible primary
 * ray provably misses the scene's root box and every light (outside all of
 * pt_primary_cull_rects' rectangles) is not ray-generated: each of its samples
 * is (0,0,0) exactly as the reference computes it (pre-pass misses, depth-0
 * traceRay misses, background 0).  0 = generate and trace every sample.
 * Path-recursive and wavefront kernels; output is identical either way. */
#define PT_OPT_PRIMARY_CULL 6
/* PT_OPT_WF_PATHS: wavefront kernel only — paths (pixel x sample) held in
 * device memory per chunk; 0 = 2^27 (56 GB; halved until the allocation
 * succeeds).  A launch with more runs in chunks of whole batches (at least
 * one batch of the frame per chunk).
 * Output is identical for every value. */
#define PT_OPT_WF_PATHS 7
/* PT_OPT_ITEM_ORDER: 1 = live items (tile parts) launched heaviest first by
 * a host estimate (pixels inside the root box's rectangle), so long
 * workgroups start early and short ones fill the tail; 0 = scan order; -1
 * (default) = auto: scan order for a whole frame on the path-recursive
 * kernel, heaviest first on a share of the frame and on the wavefront
 * pipeline.  The packed exchange layout follows the same order.  Output is
 * identical. */
#define PT_OPT_ITEM_ORDER 8
/* PT_OPT_LAUNCH_TIMING: record a HIP event pair around every k-th render
 * launch (0 = none, the default since ABI 3: on one stream a pair cost the box
 * frame ~10 us of its ~0.25 ms) for pt_last_launch_ms / pt_launch_times_ms /
 * pt_launch_span_ms.  Output-invariant. */
#define PT_OPT_LAUNCH_TIMING 9
/* PT_OPT_COUNT_TRACED: 1 = run the fast kernels with counters of the work
 * they actually do (pt_get_traced); slower, output identical.  Default 0.
 * The counting kernels always run the threaded walk: with the sweep walk in
 * force (PT_OPT_SMALL_SWEEP) the counts are still the threaded walk's node
 * visits and triangle tests, not the sweep's box tests. */
#define PT_OPT_COUNT_TRACED 10
/* PT_OPT_PAIRS: 0 only.  1 (child-pair records, measured slower on every
 * scene) was removed: PT_ERR_UNSUPPORTED. */
#define PT_OPT_PAIRS 11
/* PT_OPT_WIDE: 1 (default) = the wavefront pipeline walks device-memory
 * scenes over a 4-wide BVH of the reference's own boxes, nearest child first,
 * culling children that cannot hold a hit at or before the best one found
 * (the bound is exact-safe for the shader's float
 * Moller-Trumbore, so every hit is the exhaustive DFS's bit for bit).  Built
 * at upload when the tree's boxes contain their subtrees (any
 * BoundingVolumeHierarchy.cpp tree does); pt_wide_info reports it.  0 = the
 * threaded exhaustive walk; 2 = the wide walk with every odd ray of each
 * round handed to the exact walk (tests the hand-back path).  Output is
 * identical. */
#define PT_OPT_WIDE 12
/* PT_OPT_WF_STREAMS: 2 = the wavefront pipeline runs a chunk's pixels as
 * two halves on the context's stream and a second stream of its own (forked
 * from and joined back into the context's stream), so one half's trace and
 * shading can fill the other's launch tails; 1 (default; 2 measured slower
 * on the random clouds) = one stream.  Output is identical. */
#define PT_OPT_WF_STREAMS 13
/* PT_OPT_WIDE_BUILD (read by pt_upload_scene): how the culled wide walk's
 * 4-wide nodes group the reference's leaves.  1 (default) = a binned-SAH tree
 * over the reference's leaf boxes; 0 = the reference's own tree collapsed to
 * 4-wide nodes.  Every child box is a reference leaf box bitwise or contains
 * the leaf boxes below it, so the walk's answers are the same. */
#define PT_OPT_WIDE_BUILD 14
/* PT_OPT_WF_FUSE: 1 (default) = with the culled wide walk, a lane of the
 * wavefront traversal kernel that finds a closest hit for a primary, bounce
 * or SSS ray also samples the path's first light (the draws pathTrace makes
 * next, raytrace_comp.comp:345-366 / :383-402) and walks that shadow ray
 * itself, so the path skips a ray round; the shading kernel takes both
 * answers and runs the same shading.  0 = one ray per round.  Output is
 * identical. */
#define PT_OPT_WF_FUSE 15
/* PT_OPT_WIDE_NODE: byte size of the culled wide walk's nodes.  64 (default)
 * = child boxes rounded outward onto an 8-bit grid per node (half the bytes
 * and load instructions per node visit; a leaf's exact box is tested before
 * its hit counts); 128 = the boxes as floats.  Both are built at upload.
 * Output is identical.  80 (8-wide nodes, measured slower) was removed:
 * PT_ERR_UNSUPPORTED. */
#define PT_OPT_WIDE_NODE 16
/* PT_OPT_WF_TAIL: with the culled wide walk (4-wide nodes), once a ray
 * round's list holds fewer than this many rays, one persistent launch runs
 * every remaining path to its end (each lane walks a ray, shades it and walks
 * the path's next ray) instead of a trace and a shading launch per remaining
 * round; 0 = never; -1 (default) = auto (400000 rays).  Output is
 * identical. */
#define PT_OPT_WF_TAIL 17
/* PT_OPT_GROUP_EXCHANGE (pt_create_multi contexts only): 0 (default) = each
 * member stores its tiles straight into the frame on the first device (peer
 * access over xGMI) when every member can map it, else packed copies; 1 =
 * always packed copies (pt_tiles_pack, hipMemcpyPeerAsync, pt_tiles_unpack).
 * Output is identical. */
#define PT_OPT_GROUP_EXCHANGE 18
/* PT_OPT_GROUP_CHECK (pt_create_multi contexts only): before peer stores
 * carry a frame, a probe frame (16n x 32 pixels, 1 spp) is rendered once
 * through peer stores and once through the staged exchange, and the two are
 * compared bit for bit; on any difference the context falls back to the
 * staged exchange for good (pt_group_check reports it).  1 (default) = once
 * per context, when its members span distinct devices; 2 = on the first
 * render after every pt_resize_and_clear / pt_bind_accum, any devices; 3 =
 * as 2 with a mismatch forced (tests of the fallback); 0 = never. */
#define PT_OPT_GROUP_CHECK 19
/* PT_OPT_WF_GRID: wavefront traversal launches use this percentage (1-100,
 * default 100) of a full-occupancy persistent grid; with frames in flight on
 * several contexts a smaller grid gives each lane more rays per round.
 * Output is identical. */
#define PT_OPT_WF_GRID 20
/* PT_OPT_WF_REFILL: idle lanes at which a wave of the wavefront's wide
 * traversal kernel claims new rays; 0 (default) = auto: 16 with a full grid,
 * 8 with PT_OPT_WF_GRID below 100.  Output is identical. */
#define PT_OPT_WF_REFILL 21
/* PT_OPT_MIXED_LANES: one-rank path-recursive launches of LDS-resident scenes
 * (box.obj) with primary culling mix lane counts per workgroup: whole 16x16
 * tiles at one lane per pixel (all samples of a pixel in one lane: the least
 * work per sample, the longest workgroups) and tile parts at more lanes
 * (short workgroups that fill the launch's drain).  -1 (default) = measured:
 * until the frame's inputs have been measured, every item runs at
 * PT_OPT_SAMPLE_LANES (uniform lanes); render_kernel meanwhile times its
 * blocks (two launches once the inputs are unchanged for a render, copied
 * back without a host wait), and from then on every wholly live tile runs as
 * two 16x8 halves at 2 lanes per pixel and the live parts of the other tiles
 * at PT_OPT_SAMPLE_LANES, all items longest first by their measured cost
 * (pt_mixed_info reports the schedule).  A change of
 * size, batches, camera, params, scene or lights starts over.  k = 1-1000:
 * the static schedule with whole tiles for k % of the resident workgroups,
 * never measured.  0 = off (every item at PT_OPT_SAMPLE_LANES).  Output is
 * identical for every value. */
#define PT_OPT_MIXED_LANES 22
/* PT_OPT_DENOISE_LDS: 1 (default) = pt_denoise's passes at tap spacing 1 and
 * 2 stage their 16x16 tile and its halo in LDS; 0 = every tap is read from
 * the images.  At 1080p the staged passes measured 0.1170 / 0.1095 ms against
 * 0.1210 / 0.1124 ms, the 5-pass call 0.6430 against 0.6502 ms
 * (profiles/denoise/timing_1080p.json).  Output is identical. */
#define PT_OPT_DENOISE_LDS 23
/* PT_OPT_SMALL_SWEEP: a scene of at most 32 triangles, staged in LDS
 * (PT_OPT_SCENE_IN_LDS), can be walked by the path-recursive kernel as a
 * wave-uniform sweep: one slab test per distinct node box, read through the
 * scalar cache, then per leaf a mask test "its box and every ancestor's box
 * passed", then the triangle tests in visit order.  The slab test is pure and
 * culls nothing by distance, so the candidates, their order and every hit are
 * the threaded walk's bit for bit.  -1 (default) = the sweep
 * for scenes of at most 15 distinct boxes, the largest size at which it
 * measured no slower than the threaded walk by mean and by fastest launch
 * (box.obj has 7: 1080p 8 spp 0.192 -> 0.159 ms per frame; profiles/sweep/);
 * 1 = the sweep for every scene of at most 32 triangles (63 boxes: +70 %);
 * 0 = the threaded walk.
 * pt_sweep_info reports whether the sweep is in force.  Stats mode and
 * PT_OPT_COUNT_TRACED run the threaded walk either way.  Output is
 * identical. */
#define PT_OPT_SMALL_SWEEP 24
/* PT_OPT_SWEEP_HULL: the sweep table marks each flat box that is a face of
 * the root box (its flat coordinate bitwise the root's lo or hi on that axis,
 * its other four extents bitwise the root's: box.obj's six), and the walk
 * tests such a box with the slab products the root's test has just formed
 * instead of computing them again -- the same operands through the same
 * operations, so the same bits.  1 (default) = on; 0 = the
 * walk reads a table without the marks.  Output is identical. */
#define PT_OPT_SWEEP_HULL 26
/* PT_OPT_MOMENTS: 1 = renders also fold the per-pixel luminance moments
 * (above) with the MOMENTS instantiations of the render and fold kernels; 0
 * (default) = off, the kernels and frames of before.  The accumulator is the
 * same bits either way. */
#define PT_OPT_MOMENTS 27
/* PT_OPT_CULL_TIGHT: beside the primary-culling rectangles, which hold for
 * every Box-Muller radius (at most 13.23), the host derives a second set for
 * radii of at most 4.25 (pt_primary_cull_rects_r).  A pixel inside the first
 * set but outside the second -- the margin of aperture parallax and jitter
 * around every object -- can reach the scene or a light only with a radius
 * above 4.25, which a draw has with probability 1.2e-4.  render_kernel makes
 * a sample's four draws first and traces it for such a pixel only if one of
 * the two radius draws is below the threshold; otherwise the sample is
 * (0,0,0), which is what the trace would return.  1 (default)
 * = on; 0 = every sample of a live pixel is traced.  Needs
 * PT_OPT_PRIMARY_CULL; stats mode never skips.  Output is identical. */
#define PT_OPT_CULL_TIGHT 25
/* PT_OPT_EXIT_SKIP: 1 (default) = after a hit whose stored normal is
 * axis-pure (two components +-0, the third of magnitude 0.999 to 2) at a point
 * that lies, offset along the normal, beyond the root box's face on that side,
 * the fast kernels end the path instead of sampling and tracing its bounce
 * ray: the ray's component on that axis has the normal's sign for every
 * hemisphere draw below 1, so the reference's root-box test fails and the
 * path adds (0,0,0) (box.obj's outward faces).  In force
 * only when some triangle of the scene has such a normal and every light's
 * intensity is finite; stats mode never skips.  Output is identical;
 * PT_OPT_COUNT_TRACED counts the walks not started. */
#define PT_OPT_EXIT_SKIP 28
/* PT_OPT_SEED_BASE: B = 0 (default) to 2^31-1.  The sample of batch b is drawn
 * from the seed ((b + B) * H + py) * W + px (uint32 arithmetic) instead of
 * (b * H + py) * W + px, and still folded into the accumulator and the moments
 * with weight b: a frame rendered from batch 0 with fresh random numbers.  The
 * shader ties the seed to the fold weight, so every frame from batch 0 repeats
 * its numbers per pixel, and frames averaged over time would add little.
 * Every render path (multi-device contexts forward it).  0: the frames of
 * before. */
#define PT_OPT_SEED_BASE 29
/* PT_OPT_SWEEP_CUBE: a sweep table in which every box other than the root is
 * a hull face of it (PT_OPT_SWEEP_HULL; no general box, no uncoded flat box:
 * box.obj, a cuboid, a cuboid without some face) is walked by a straight-line
 * kernel: the root's six slab products, its test, the one ballot, then the six
 * faces with their axis and side fixed at compile time, their leaf masks and
 * the root box taken from the kernel's parameters -- no loop over the table
 * and no record load.  The same booleans from the same operands as the hull
 * walk, so the same bits.  1 (default) = on; 0 = the
 * hull walk.  A table with any other box runs the hull walk either way;
 * pt_sweep_walk tells which walk is in force.  Output is identical. */
#define PT_OPT_SWEEP_CUBE 30
/* PT_OPT_ADAPTIVE_WF: 1 = pt_adaptive_begin / pt_adaptive_advance run their
 * rounds on the wavefront pipeline when PT_OPT_KERNEL is 0 or 3 (1, the
 * explicit request for the path-recursive kernel, wins): every live tile's
 * paths of the round in the path buffers, traced by the kernels pt_render's
 * wavefront launches run -- the culled wide walk for a scene that has one and
 * is not staged in LDS -- under the same options (PT_OPT_WIDE, PT_OPT_WIDE_NODE,
 * PT_OPT_WF_FUSE, PT_OPT_WF_TAIL, PT_OPT_WF_REFILL, PT_OPT_WF_GRID,
 * PT_OPT_WF_PATHS, PT_OPT_EXIT_SKIP, PT_OPT_SCENE_IN_LDS); PT_OPT_WF_STREAMS 2
 * is not used by the rounds.  pt_last_kernel then reports 3 after
 * pt_adaptive_begin.  0 (default) = the path-recursive rounds, and
 * PT_OPT_KERNEL 3 is refused by the adaptive calls.  Every other refusal of the
 * adaptive calls holds either way.  Output is identical: counts, live lists,
 * accumulation image and moments. */
#define PT_OPT_ADAPTIVE_WF 31
/* PT_OPT_RAYS_REFILL: the shape of pt_trace_rays' culled wide walk.  1 = a
 * persistent grid whose lanes refill singly from a ray counter once
 * PT_OPT_WF_REFILL lanes of their wave are idle, leaf queues tested across the
 * wave (the wavefront trace kernel's shape); 0 = one ray per lane to its end,
 * then the next by a grid stride, leaf queues tested per lane (the guide
 * kernel's shape).  1 is the default: on
 * 2M incoherent rays it measured 34 % (closest) and 26 % (occlusion) less time
 * on a 20,480-triangle sphere and 33 % and 24 % less on a 10M-triangle cloud;
 * on the coherent rays of a 1080p frame 0 took 14 % less on the sphere and 10 %
 * more on the cloud (profiles/rays/timing.json).  Output is identical. */
#define PT_OPT_RAYS_REFILL 32
/* PT_OPT_CULL_FOOTPRINT: the per-sample skip of PT_OPT_CULL_TIGHT decides by
 * footprints instead of the tight rectangles (pt_primary_cull_footprints): per
 * object a convex region inside its tight rectangle -- every corner dilated by
 * its own depth against the focal depths of the rays that can reach the
 * object, and the hull of the results cut out of the rectangle by up to four
 * half-planes.  A live pixel outside every footprint traces a sample only if
 * one of its two radius draws is below the threshold, exactly as a pixel
 * outside every tight rectangle does; there are more such pixels.  A pixel in
 * a light's sure region (pt_primary_cull_sure) and in no footprint but that
 * light's own takes (intensity, 1) for such samples instead of (0,0,0).  -1
 * (default) = on, but off while PT_OPT_COUNT_TRACED is set: the counting pass
 * then keeps the rectangle definition above, counts the margin samples by the
 * rectangles, and so reports somewhat more primaries and closest walks than
 * the fast kernel starts.  1 = on in counting mode too; 0 = off, the tight
 * rectangles decide.  Off whenever PT_OPT_PRIMARY_CULL or PT_OPT_CULL_TIGHT
 * is; stats mode never skips.  pt_cull_info reports what is in force.  Output
 * is identical. */
#define PT_OPT_CULL_FOOTPRINT 33
/* PT_OPT_RADIANCE_CHUNK: the paths (queries x samples) pt_trace_radiance runs
 * in one chunk; a chunk holds whole queries, at least one.  0 (default) = auto,
 * 2^22 paths: 64 MiB of colours on the path-recursive kernel, 1.7 GB of path
 * state (416 B a path) on the wavefront pipeline, and one chunk for the rays of
 * a 1080p frame.  Output is identical; small values exist so that tests reach
 * chunk seams with few queries. */
#define PT_OPT_RADIANCE_CHUNK 34
int pt_set_option(pt_context* ctx, int key, int value);
/* The kernel the last pt_render / pt_dispatch ran (PT_OPT_KERNEL values 1-3,
 * after auto selection); 0 before the first render. */
int pt_last_kernel(pt_context* ctx, int* kernel);

/* Screen regions that primary rays can reach the scene or a light from.
 * Writes up to max_rects NDC rectangles {x0, x1, y0, y1} (one per object:
 * the root box, then each light) to rects and their count to *n_rects; a
 * pixel whose (2px/W - 1, 2py/H - 1) lies outside all of them has no primary
 * ray (any aperture draw, any jitter draw — Box-Muller radii are bounded by
 * 13.23 since u1 >= 1e-38, raytrace_comp.comp:220) that hits the root box or
 * a light.  *n_rects = -1 when no such guarantee is derived (object at or
 * behind the camera plane, degenerate camera, more lights than max_rects-1):
 * every pixel is then traced.  Pure host function. */
int pt_primary_cull_rects(const float camera_ubo[16], int width, int height, const float root_min[3],
                          const float root_max[3], const pt_area_light* lights, int n_lights, float* rects,
                          int max_rects, int* n_rects);
/* The same derivation for samples whose two Box-Muller radii are at most
 * radius_bound (0 to 13.25; negative = the kernel's tight bound, 4.25): outside
 * the rectangles no primary ray with such radii hits the root box or a light.
 * The kernel derives this tight set beside the one above (PT_OPT_CULL_TIGHT)
 * and, for a pixel inside the loose set but outside the tight one, traces a
 * sample only if one of its two radius draws u1 is below *u0 -- the least
 * float for which every float u in [*u0, 1] has the kernel's
 * sqrt(-2 log(max(1e-38, u))) at most 4.25 (u0 may be null).  *n_rects = -1 as
 * above.  Pure host function. */
int pt_primary_cull_rects_r(const float camera_ubo[16], int width, int height, const float root_min[3],
                            const float root_max[3], const pt_area_light* lights, int n_lights, double radius_bound,
                            float* rects, int max_rects, int* n_rects, float* u0);
/* The footprints of the same objects for the same radius bound
 * (PT_OPT_CULL_FOOTPRINT): 16 floats each, {x0, x1, y0, y1} then four
 * half-planes {a, b, c}; a pixel origin (x, y) is inside when it is inside the
 * rectangle and a * x + b * y <= c in float arithmetic for all four (an unused
 * half-plane is {0, 0, 1}).  Outside every footprint no primary ray with such
 * radii hits the root box or a light.  Each footprint lies inside the
 * rectangle pt_primary_cull_rects_r gives its object for the same bound.
 * *n_footprints = -1 as above (the kernel then goes by the rectangles).  Pure
 * host function. */
int pt_primary_cull_footprints(const float camera_ubo[16], int width, int height, const float root_min[3],
                               const float root_max[3], const pt_area_light* lights, int n_lights,
                               double radius_bound, float* footprints, int max_footprints, int* n_footprints);
/* The sure regions for the same bound, one per light, in a footprint's layout
 * (an empty one, x0 > x1, where none is derived: a non-finite intensity, a
 * size component that is not positive -- intersectAreaLight never hits such
 * a light -- a light seen nearly edge-on, a corner behind the camera).  Every primary ray
 * with such radii from a pixel inside a light's region hits that light; where
 * the pixel also lies outside the footprint of the root box and of every
 * other light, the sample is exactly (intensity, 1).  *n_sure = the number of
 * non-empty regions, or -1 when there are no footprints.  Pure host function. */
int pt_primary_cull_sure(const float camera_ubo[16], int width, int height, const float root_min[3],
                         const float root_max[3], const pt_area_light* lights, int n_lights, double radius_bound,
                         float* regions, int max_regions, int* n_sure);
/* What the per-sample skip of the context's next launch decides by, as its
 * camera, size, scene, lights and options stand: info[0] = tight rectangles,
 * info[1] = footprints among them (0: the rectangles alone decide), info[2] =
 * non-empty sure regions.  Zeros when nothing is derived or the skip is off. */
int pt_cull_info(pt_context* ctx, int info[3]);

/* ---- instrumentation --------------------------------------------------- */
/* Stats mode runs the reference-exhaustive traversal with counters (output is
 * unchanged); used for the roofline's algorithmic byte count. */
int pt_set_stats_mode(pt_context* ctx, int enabled);
int pt_get_stats(pt_context* ctx, pt_stats* out);
int pt_reset_stats(pt_context* ctx);
int pt_get_traced(pt_context* ctx, pt_traced* out);
/* The culled wide walk of the uploaded scene (PT_OPT_WIDE): info[0] = wide
 * nodes (0 = not built; pt_last_error() then says why), info[1] = the most
 * stack entries one walk can hold. */
int pt_wide_info(pt_context* ctx, int info[2]);
/* The sweep walk of the uploaded scene (PT_OPT_SMALL_SWEEP): the distinct
 * boxes and the leaves of its table when the context's launches, as its
 * options stand, walk it -- the option's value admits the scene,
 * PT_OPT_SCENE_IN_LDS is not 0, PT_OPT_KERNEL is not 3, and neither stats
 * mode nor PT_OPT_COUNT_TRACED is on (the same predicate pt_render uses) --
 * else zeros. */
int pt_sweep_info(pt_context* ctx, int* boxes, int* leaves);
/* Which walk those launches run, by the same predicate: *walk = 0 the
 * threaded walk, 1 the sweep that keeps nothing from the root's test, 2 the
 * sweep with hull faces (PT_OPT_SWEEP_HULL), 3 the straight-line sweep of a
 * cube table (PT_OPT_SWEEP_CUBE). */
int pt_sweep_walk(pt_context* ctx, int* walk);
/* Mixed sample lanes of the last path-recursive launch (PT_OPT_MIXED_LANES):
 * info[0] = 0 uniform lanes, 1 the static mixed schedule, 2 the measured one;
 * info[1] = live workgroups it launched; info[2] = measuring launches folded
 * into the current inputs' block costs.  Multi-device contexts: zeros. */
int pt_mixed_info(pt_context* ctx, int info[3]);
/* Device time of the last pt_render/pt_dispatch launch, from HIP events
 * recorded on the launch stream. */
int pt_last_launch_ms(pt_context* ctx, float* ms);
/* Device times of every render launch since pt_reset_launch_times (the last
 * 512 at most), oldest first; waits for them to finish. */
int pt_launch_times_ms(pt_context* ctx, float* out, size_t max_n, size_t* n_out);
/* Device time from the start of the first render launch since
 * pt_reset_launch_times to the end of the last one (launches on several
 * streams overlap, so their durations do not add up); *n_out = launches.
 * Waits for them to finish; PT_ERR_UNSUPPORTED past 512 launches. */
int pt_launch_span_ms(pt_context* ctx, float* ms, size_t* n_out);
int pt_reset_launch_times(pt_context* ctx);
/* Evaluates the kernel's fp32 math on the device for bitwise checks against
 * the oracle: fn 0 log, 1 exp, 2 sin, 3 cos, 4 tan, 5 acos, 6 sqrt,
 * 7 first RNG draw from the seed given as the float's bits, 8 reciprocal. */
int pt_selftest_math(int device_ordinal, int fn, const float* x, float* y, size_t n);
/* Exhaustive check of the device's fast-quotient math against its IEEE
 * definitions over all 2^32 inputs: fn 0 rcp (1/x), 1 log, 2 exp, 3 acos.
 * The wave-uniform fast forms on their pieces (an input inside the form's
 * range must give the IEEE bits from the unguarded form): fn 4 sqrt, 5 rcp,
 * 7 x / 1.5f; fn 6 sincos against sin and cos, both results.
 * Writes the number of differing inputs and the smallest such
 * input's bit pattern (0xffffffff if none). */
int pt_selftest_exhaustive(int device, int fn, unsigned long long* mismatches, uint32_t* first_bad);

/* ---- host scene layer (L1 producers: BVH, Light, OBJ ingest) ----------- */
typedef struct pt_scene pt_scene;
/* tinyobj::ObjReader::ParseFromFile + index gathering (VulkanRayTracer.cpp:64-92) */
int pt_scene_load_obj(const char* path, pt_scene** out);
int pt_scene_parse_obj(const char* text, size_t len, pt_scene** out);
/* scene from raw arrays (e.g. synthetic meshes) */
int pt_scene_from_arrays(const float* vertices, size_t n_vertex_floats,
                         const uint32_t* indices, size_t n_indices, pt_scene** out);
/* BVH bvh(objVertices, objIndices) (BoundingVolumeHierarchy.cpp:5-23);
 * flags: PT_NODES_INT_BITS; threads 0 = all cores. */
int pt_scene_build_bvh(pt_scene* scene, uint32_t flags, int threads);
int pt_scene_counts(const pt_scene* scene, size_t* n_vertex_floats, size_t* n_indices,
                    size_t* n_nodes, size_t* n_uv_floats, size_t* n_mat);
int pt_scene_copy(const pt_scene* scene, float* vertices, uint32_t* indices, pt_bvh_node* nodes,
                  float* uvs, uint32_t* mat_indices);
int pt_scene_upload(pt_context* ctx, const pt_scene* scene);
int pt_scene_free(pt_scene* scene);
/* Binary scene cache (skip OBJ parse + BVH build for large
 * meshes): everything pt_scene_copy returns, with an FNV-1a checksum.  Load
 * fails with PT_ERR_IO on a missing, foreign, truncated or corrupt file. */
int pt_scene_save(const pt_scene* scene, const char* path);
int pt_scene_load_cache(const char* path, pt_scene** out);
/* Light lights(positions, normals, intensities, sizes) packing (Light.cpp:16-33) */
int pt_pack_light(const float position[3], const float normal[3], const float intensity[3],
                  const float size[2], pt_area_light* out);
/* Writes a W x H RGBA32F accumulation image (row y = 0 first in memory) for
 * inspection: PT_IMAGE_PFM = float RGB PFM (rows
 * bottom-to-top, i.e. row 0 first); PT_IMAGE_PNG = 8-bit sRGB PNG of the
 * colours clamped to [0,1], top row = last buffer row. */
#define PT_IMAGE_PFM 0
#define PT_IMAGE_PNG 1
int pt_write_image(const char* path, const float* rgba, int width, int height, int format);
/* Writes W x H RGBA8 pixels (pt_read_display's) as the same PNG: top row = last
 * buffer row, alpha dropped.  Of pt_display's bytes at the default parameters
 * it is the file pt_write_image(PT_IMAGE_PNG) writes of the floats. */
int pt_write_png8(const char* path, const unsigned char* rgba8, int width, int height);
/* Camera getters for the reference's default orbit camera, as the UBO
 * (Camera.cpp:4-10, 84-106): pos (0,0,5) dir (0,0,-1) up (0,1,0) fov 60. */
int pt_default_camera(float camera_ubo[16]);

#ifdef __cplusplus
}
#endif
#endif /* PATHTRACER_H_ */
