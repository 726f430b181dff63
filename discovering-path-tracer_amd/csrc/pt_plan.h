// pt_plan.h — internal: the launch plan.  Every policy of the library -- which
// kernel a frame runs on, with how many sample lanes, staged in LDS or not,
// walked by which walk, in which item order -- is decided by plan_launch, a pure
// function of the context: it writes nothing, calls no HIP function and
// allocates nothing, so a stand-alone host program can table-test it
// (tests/plan_check.cpp, tests/plan_cases.py).  render_impl (pt_api.cpp) carries
// the plan out; pt_sweep_info and pt_render_guide answer from the same rules.
#pragma once
#include <stdint.h>

#include <cmath>

#include "pt_context.h"

#pragma GCC visibility push(hidden)

// The sweep walk's enabling bound (PT_OPT_SMALL_SWEEP -1, the default): a
// scene that has a sweep table (at most pt::kSweepMaxLeaves triangles) is
// walked by it when the table holds at most this many distinct boxes -- the
// largest size at which the sweep did not lose to the threaded walk by the
// mean and by the fastest launch alike (profiles/sweep/sweep_sizes.log,
// 512x512 8 spp, on / off by mean and by minimum: 7 boxes 0.79-0.94 and
// 0.78-0.97, 15 boxes 0.98 and 0.96; 21 boxes 0.79 by the mean but 1.04 by
// the minimum, the threaded walk's launches scattering widely there; 31
// boxes 1.11-1.17 and 1.18-1.22, 63 boxes 1.68 and 1.72).  The slab tests set
// the cost: 32 leaves over 31 boxes lose like 16 leaves over 31.
constexpr int kSweepAutoBoxes = 15;

constexpr int kWfAutoTris = 32768;
constexpr int kWfWideAutoTris = 16384;   // ... with the culled wide walk (plan_launch)

// Whether the context's launches walk the scene's sweep table (PT_OPT_SMALL_SWEEP): the
// option admits the scene, and the launch is the plain LDS-staged path-recursive kernel
// (a scene with a table always fits in LDS; the auto kernel choice is path-recursive for it).
inline bool sweep_in_force(const pt_context* c) {
  const bool wanted =
      c->d_sweep && (c->opt_small_sweep == 1 || (c->opt_small_sweep < 0 && c->sweep_boxes <= kSweepAutoBoxes));
  return wanted && c->opt_scene_lds != 0 && c->opt_kernel != 3 && !c->stats_mode && c->opt_count == 0;
}

// Which sweep walk those launches run (pt_sweep_walk): 1 the walk that keeps nothing from the root's
// test, 2 the one that tests hull faces with the root's products (PT_OPT_SWEEP_HULL, a table that has
// some), 3 the straight-line walk of a cube table (PT_OPT_SWEEP_CUBE): a hull table with no other box.
// A hull table that also has a general or an uncoded box stays on 2.
inline int sweep_walk_kind(const pt_context& c) {
  if (!c.opt_sweep_hull || c.sweep_hull <= 0) return 1;
  return c.opt_sweep_cube && c.sweep_cube ? 3 : 2;
}

// The LDS rule (PT_OPT_SCENE_IN_LDS) of a scene of n_nodes threaded nodes: 2 asks for the LDS
// variant and is refused when the scene cannot fit, 1 stages a scene that fits, 0 none.
constexpr const char* kLdsTooLarge = "scene too large for the LDS variant";
inline bool lds_fits(const pt_context& c, int n_nodes) {
  ptd::RenderParams s{};
  s.n_nodes = n_nodes;
  s.n_tris = c.n_tris;
  return ptd::scene_lds_bytes(s) <= ptd::kMaxSceneLds;
}
inline bool lds_refused(const pt_context& c, bool fits) { return c.opt_scene_lds == 2 && !fits; }
inline bool lds_staged(const pt_context& c, bool fits) {
  return c.opt_scene_lds == 2 || (c.opt_scene_lds == 1 && fits);
}

// The culled wide walk's node layout (PT_OPT_WIDE_NODE): 1 = the 64-B nodes.
inline int wide_layout_qn(const pt_context& c) { return c.opt_wide_node == 64 ? 1 : 0; }

struct LaunchPlan {
  // PT_OK / nullptr, or what the render is refused with (a string literal).  The moments refusals
  // come before the render touches anything (refuse_first); the others after its bookkeeping has
  // opened (render_impl).
  int refuse_code = PT_OK;
  const char* refuse = nullptr;
  bool refuse_first = false;
  int spl = 0;                  // sample lanes per pixel
  bool lds = false;             // the scene is staged in LDS
  bool wf = false;              // the wavefront pipeline (else the path-recursive kernel)
  bool cnt = false;             // traced-work counters (PT_OPT_COUNT_TRACED)
  bool sweep = false;           // the sweep walk ...
  bool sweep_hull = false;      // ... reading the table with hull codes, and finding some
  bool sweep_cube = false;      // ... all of whose boxes but the root are hull faces: the straight-line walk
  bool wide = false;            // the wavefront pipeline's culled wide walk
  bool mixed_eligible = false;  // mixed lanes, if the frame has cull rectangles
  int item_order = 0, exit_skip = 0;
  int wide_qn = 0, wide_handback = 0, wf_fuse = 0, wf_tail = 0;   // of the wide walk (0 without it)
  int wide_refill = 0;
  bool two_streams = false;     // the wavefront pipeline's second stream
};

// The plan of the render of n_batches batches over this rank's n_tiles tiles (packed: pt_render_packed,
// a pt_dist_run frame).  kernel: the kernel asked for where the caller's own option overrides PT_OPT_KERNEL
// (plan_adaptive under PT_OPT_ADAPTIVE_WF), -1 = the option's.
inline LaunchPlan plan_launch(const pt_context& c, long long n_tiles, uint32_t n_batches, bool packed,
                              int kernel = -1) {
  LaunchPlan pl;
  auto refuse = [&pl](const char* msg, bool first) {
    if (pl.refuse) return;   // the first refusal is the one reported
    pl.refuse_code = PT_ERR_UNSUPPORTED;
    pl.refuse = msg;
    pl.refuse_first = first;
  };
  if (c.opt_moments) {
    if (packed) refuse("PT_OPT_MOMENTS: not with pt_render_packed or pt_dist_run", true);
    if (c.nranks > 1) refuse("PT_OPT_MOMENTS: not on a partition of more than one rank", true);
    if (c.stats_mode) refuse("PT_OPT_MOMENTS: not in stats mode", true);
    if (c.opt_count) refuse("PT_OPT_MOMENTS: not with PT_OPT_COUNT_TRACED", true);
  }
  // PT_OPT_WF_REFILL auto: 16 idle lanes on a full grid, 8 on a split one
  // (more rays per lane per round; the refill's cost is shared by fewer
  // concurrent waves: profiles/r05i)
  pl.wide_refill = c.opt_wf_refill > 0 ? c.opt_wf_refill : (c.opt_wf_grid < 100 ? 8 : 16);
  // the exit skip (PT_OPT_EXIT_SKIP): only where it can fire and rad is finite
  pl.exit_skip = c.opt_exit_skip && c.exit_normals && !c.stats_mode ? 1 : 0;
  for (int i = 0; i < c.n_lights && pl.exit_skip; ++i)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(c.lights_host[(size_t)i].intensity[k])) pl.exit_skip = 0;
  const bool fits = lds_fits(c, c.stats_mode ? c.n_nodes_full : c.n_nodes);
  if (c.opt_sample_lanes) {
    pl.spl = c.opt_sample_lanes;
  } else {
    // auto: 4 sample lanes per pixel for an LDS-resident scene on up to 7
    // ranks, else 8 — on a share of the frame each GPU's share shrinks while
    // its heaviest workgroup does not, and on big scenes the samples of one
    // pixel walk nearly the same nodes, so their loads coalesce.  Measured
    // at 1080p 8spp with culling and compact launch: box spl 1/2/4/8 =
    // 0.499/0.408/0.375/0.416 ms (whole frame), 0.354/0.264/0.225/0.221
    // (1/2), 0.271/0.156/0.094/0.085 (1/8); displaced sphere 828/645/582/563;
    // 1M cloud 968/930/927/923.  Never more lanes than samples.
    // With frames alternating between two streams (bench.py N > 1), the
    // 1/2 and 1/4 shares favour 4 lanes (0.187 vs 0.210, 0.101 vs 0.110 ms
    // per step) and the 1/8 share 8 (0.062 vs 0.069).  Round 3's kernels,
    // the emulated root step on the native loop (DESIGN Appendix A, round-3 share options;
    // two runs each): 1/2 share spl 2/4 = 0.1175/0.1225 ms, 1/4 share 4/8 =
    // 0.069/0.082, 1/8 share 4/8 = 0.046/0.042.  Round 5's kernels (the
    // build without the SLP vectorizer, profiles/r05zc/spl.log, 200 frames):
    // 1/2 share spl 1/2/4/8 = 0.1066/0.1067/0.118/0.1411 ms, 1/4 share
    // 0.0811/0.0594/0.0603/0.0692, 1/8 share 0.0725/0.0465/0.0348/0.0374.
    int want = !fits ? 8 : c.nranks >= 8 ? 4 : c.nranks >= 2 ? 2 : 4;
    while (want > 1 && (uint32_t)want > n_batches) want >>= 1;
    pl.spl = want;
  }
  if (lds_refused(c, fits)) refuse(kLdsTooLarge, false);
  pl.lds = lds_staged(c, fits);
  // auto: the wavefront pipeline for scenes of at least kWfAutoTris triangles
  // (not LDS-resident) when the launch holds enough paths to keep its node
  // loads in flight, the path-recursive kernel otherwise.  Measured at 1080p
  // (ms, recursive with paired walks -> wavefront): 1 spp (2M paths):
  // displaced sphere 82K tris 101 -> 108, 10M cloud 735 -> 669; 8 spp (16.6M):
  // sphere 550 -> 465, 100K cloud 113 -> 77; 1M cloud 2 spp 225 -> 236; a 1/8
  // tile share of the 10M cloud: 1 spp (259K paths) 147 -> 273, 8 spp (2M)
  // 742 -> 669; box 0.38 -> 8.4.
  // With the culled wide walk (PT_OPT_WIDE) the wavefront pipeline wins from
  // 2^20 paths on (1080p, ms recursive -> wavefront): displaced sphere 82K
  // 1 spp 89.9 -> 39.6, 8 spp 498 -> 139, its 1/8 tile share 89.0 -> 39.1;
  // 20K sphere 2 spp 29.6 -> 23.3; 1M cloud 1 spp 108 -> 47.5; a sparse 100K
  // cloud at 1 spp (most rays miss) loses 14.3 -> 15.9.
  const long long paths = (long long)n_tiles * 256 * n_batches;
  const bool wide_walk = c.opt_wide && c.n_wide > 0;
  const bool wf_auto = wide_walk ? c.n_tris >= kWfWideAutoTris && paths >= (1ll << 20)
                                 : c.n_tris >= kWfAutoTris && paths >= (1ll << 20) &&
                                       (c.n_tris >= (1 << 20) || paths >= (1ll << 23));
  const int asked = kernel < 0 ? c.opt_kernel : kernel;
  pl.wf = asked == 3 || (asked == 0 && !pl.lds && !c.stats_mode && wf_auto);
  if (pl.wf && c.stats_mode) refuse("stats mode runs the path-recursive kernel only", false);
  pl.cnt = c.opt_count != 0 && !c.stats_mode;
  // the sweep walk (PT_OPT_SMALL_SWEEP): the plain LDS kernel of a scene with a table
  pl.sweep = pl.lds && !pl.wf && !pl.cnt && sweep_in_force(&c);
  const int walk = pl.sweep ? sweep_walk_kind(c) : 0;
  pl.sweep_hull = walk >= 2;
  pl.sweep_cube = walk == 3;
  // PT_OPT_ITEM_ORDER auto: scan order for a whole frame on the path-recursive
  // kernel (box 1080p8 at 4 lanes, one context: 0.2403 against 0.2463 ms
  // heaviest first, profiles/r06b), heaviest first on a share of the frame
  // and on the wavefront pipeline
  pl.item_order = c.opt_item_order >= 0 ? c.opt_item_order : (!pl.wf && c.nranks == 1 ? 0 : 1);
  // mixed lanes (PT_OPT_MIXED_LANES): one rank, LDS-staged path-recursive
  // launches that render into the accumulation buffer
  // (one lane per pixel: the measured schedule only orders whole tiles)
  pl.mixed_eligible = c.opt_mixed != 0 && !pl.wf && pl.lds && c.nranks == 1 && !packed &&
                      (pl.spl > 1 || c.opt_mixed < 0) && !pl.cnt;
  pl.wide = pl.wf && c.opt_wide && c.n_wide > 0 && !pl.lds;
  if (pl.wide) {
    pl.wide_qn = wide_layout_qn(c);
    pl.wide_handback = c.opt_wide == 2 ? 1 : 0;
    // fused shadow walks: hit records carry the rank in 29 bits
    pl.wf_fuse = c.opt_wf_fuse && c.n_tris <= ptd::kHitRankMask && c.n_lights > 0 ? 1 : 0;
    // wf_tail_kernel (4-wide layouts).  Auto: once a list holds fewer than
    // 400K rays (with the wave-wide flush, item 39; ab_bench device time):
    // emulated 1/8 tile shares of configs 3 / 4 / 5 13.48 -> 11.31, 64.68 ->
    // 64.26, 22.36 -> 21.91 ms; whole frames 44.28 -> 43.77, 384.41 ->
    // 384.89, 117.72 -> 117.39 ms.  (2^20: 11.17 / 65.31 / 22.39; from the
    // first list: +28-57 % on whole frames.)
    const int tail_auto = 400000;
    pl.wf_tail = c.opt_wf_tail >= 0 ? c.opt_wf_tail : tail_auto;
  }
  pl.two_streams = pl.wf && c.opt_wf_streams == 2;
  return pl;
}

// The plan of an adaptive render (pt_adaptive_begin / pt_adaptive_advance): what it refuses, the
// instantiation its rounds run, their lane counts and how many rounds can still change a count.  The
// walk, LDS and exit-skip choices are plan_launch's for a path-recursive launch; by default
// (PT_OPT_ADAPTIVE_WF 0) the wavefront pipeline is refused when asked for and never chosen under auto
// (plan_launch is asked about no tile, so no launch is ever large enough for it).  Lanes: round 0 renders
// min_batches everywhere and is planned for them, every later round for `step` -- one lane count per launch,
// never more lanes than samples.
// PT_OPT_ADAPTIVE_WF 1: the rounds run on the wavefront pipeline (kernels/wf_adaptive.h) unless
// PT_OPT_KERNEL 1 asks for the path-recursive kernel; the wide walk's settings and the LDS staging are
// plan_launch's for a wavefront launch, so every option of the pipeline means what it means for pt_render.
// Its second stream (PT_OPT_WF_STREAMS 2) is not used: the two streams split a chunk's pixels in halves, and
// the host does not know how many pixels the round's live list holds.
constexpr const char* kAdaptiveBadParams =
    "pt_adaptive_params: 2 <= min_batches <= max_batches <= 65536, step >= 1; threshold and lum_floor finite and > 0";
struct AdaptivePlan {
  int refuse_code = PT_OK;      // PT_OK / nullptr, or what the call is refused with
  const char* refuse = nullptr;
  int spl0 = 0, spl = 0;        // sample lanes of round 0 and of the later rounds
  bool lds = false;             // the scene is staged in LDS
  int sweep = 0;                // the sweep walk (0 none, 1 plain, 2 hull, 3 cube)
  int exit_skip = 0;
  uint32_t rounds = 0;          // ceil((max_batches - min_batches) / step)
  ptd::AdaptiveVariant v = {};  // render_adaptive_kernel's instantiation
  bool wf = false;              // the rounds run on the wavefront pipeline (PT_OPT_ADAPTIVE_WF)
  bool wide = false;            // ... with the culled wide walk, and its settings (LaunchPlan's, 0 without it)
  int wide_qn = 0, wide_handback = 0, wf_fuse = 0, wf_tail = 0;
  int wide_refill = 0;
};
inline AdaptivePlan plan_adaptive(const pt_context& c, const pt_adaptive_params& a) {
  AdaptivePlan ap;
  auto refuse = [&ap](int code, const char* msg) {
    if (ap.refuse) return;
    ap.refuse_code = code;
    ap.refuse = msg;
  };
  if (!(a.min_batches >= 2u && a.max_batches >= a.min_batches && a.max_batches <= 65536u && a.step >= 1u &&
        a.threshold > 0.0f && a.threshold <= 3.40282347e38f && a.lum_floor > 0.0f && a.lum_floor <= 3.40282347e38f))
    refuse(PT_ERR_INVALID, kAdaptiveBadParams);
  if (c.group) refuse(PT_ERR_UNSUPPORTED, "adaptive sampling: not on a multi-device context (pt_create_multi)");
  if (c.nranks > 1) refuse(PT_ERR_UNSUPPORTED, "adaptive sampling: not on a partition of more than one rank");
  if (c.stats_mode) refuse(PT_ERR_UNSUPPORTED, "adaptive sampling: not in stats mode");
  if (c.opt_count) refuse(PT_ERR_UNSUPPORTED, "adaptive sampling: not with PT_OPT_COUNT_TRACED");
  if (c.opt_kernel == 3 && !c.opt_adaptive_wf)
    refuse(PT_ERR_UNSUPPORTED, "adaptive sampling: the path-recursive kernel only (PT_OPT_KERNEL 3)");
  if (!c.opt_moments) refuse(PT_ERR_INVALID, "adaptive sampling: needs PT_OPT_MOMENTS 1");
  if (ap.refuse) return ap;
  ap.wf = c.opt_adaptive_wf != 0 && c.opt_kernel != 1;   // the explicit request for the path-recursive kernel wins
  const int kernel = ap.wf ? 3 : -1;
  const LaunchPlan p0 = plan_launch(c, 0, a.min_batches, false, kernel);
  const LaunchPlan p1 = plan_launch(c, 0, a.step, false, kernel);
  if (p0.refuse) {
    refuse(p0.refuse_code, p0.refuse);
    return ap;
  }
  ap.spl0 = p0.spl;
  ap.spl = p1.spl;
  ap.lds = p0.lds;
  ap.sweep = !p0.sweep ? 0 : p0.sweep_cube ? 3 : p0.sweep_hull ? 2 : 1;
  ap.exit_skip = p0.exit_skip;
  ap.rounds = (a.max_batches - a.min_batches + a.step - 1u) / a.step;
  if (a.step > a.max_batches - a.min_batches) ap.rounds = a.max_batches > a.min_batches ? 1u : 0u;   // no overflow
  ap.v = ptd::pick_adaptive(ap.lds, ap.sweep, ap.exit_skip != 0);
  ap.wide = p0.wide;
  ap.wide_qn = p0.wide_qn;
  ap.wide_handback = p0.wide_handback;
  ap.wf_fuse = p0.wf_fuse;
  ap.wf_tail = p0.wf_tail;
  ap.wide_refill = ap.wf ? p0.wide_refill : 0;   // (plan_launch sets it for every launch)
  return ap;
}

#pragma GCC visibility pop
