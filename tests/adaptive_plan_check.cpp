// adaptive_plan_check — plan_adaptive (csrc/pt_plan.h) and the kernel selection of
// launch_render_adaptive (csrc/pt_device.h plan_render_adaptive) on the host, for
// tests/test_adaptive.py: a table of contexts and parameters with what the plan
// must say -- what it refuses and with which code, the instantiation, the lane
// counts of round 0 and of the later rounds, the rounds still possible.  Prints
// one line per row, then "ok: N rows", exit status 0; or what failed and 1.
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>

#include "pt_plan.h"

// pt_context.h's fail() refers to it; nothing here calls it
int pt_fail_internal(int code, const std::string&) { return code; }

namespace {

float4 g_table;       // stands for a sweep table: the plan asks only whether there is one
float2 g_moments;
int4 g_list;
pt_group* const kGroup = reinterpret_cast<pt_group*>(&g_table);   // only tested against null

int fails = 0;

// box.obj as the library sees it: 12 triangles, a cube table of 7 boxes, axis-pure normals, one finite light
void box(pt_context* c) {
  c->n_tris = 12;
  c->n_nodes = 23;
  c->n_nodes_full = 23;
  c->d_sweep = &g_table;
  c->sweep_boxes = 7;
  c->sweep_leaves = 12;
  c->sweep_hull = 6;
  c->sweep_cube = true;
  c->exit_normals = true;
  c->n_lights = 1;
  c->lights_host.resize(1);
  for (int k = 0; k < 3; ++k) c->lights_host[0].intensity[k] = 10.0f;
  c->opt_moments = 1;
  c->width = 72;
  c->height = 40;
}
// a scene too large for LDS and without a sweep table
void big(pt_context* c) {
  box(c);
  c->n_tris = 100000;
  c->n_nodes = 199999;
  c->n_nodes_full = 199999;
  c->d_sweep = nullptr;
  c->sweep_boxes = c->sweep_leaves = c->sweep_hull = 0;
  c->sweep_cube = false;
}

struct Want {
  int code;             // PT_OK, or the refusal's
  const char* refuse;   // a part of its text
  int lds, sweep, exit, spl0, spl;
  unsigned rounds;
};

void row(const char* name, const std::function<void(pt_context*)>& set, pt_adaptive_params a, const Want& w) {
  pt_context c;
  set(&c);
  const AdaptivePlan p = plan_adaptive(c, a);
  bool ok = p.refuse_code == w.code;
  if (w.code != PT_OK) {
    ok = ok && p.refuse && strstr(p.refuse, w.refuse);
    printf("%s: refuse_code=%d refuse=%s\n", name, p.refuse_code, p.refuse ? p.refuse : "(none)");
  } else {
    ok = ok && !p.refuse && (int)p.v.lds == w.lds && p.v.sweep == w.sweep && (int)p.v.exit == w.exit &&
         p.spl0 == w.spl0 && p.spl == w.spl && p.rounds == w.rounds && (int)p.lds == w.lds &&
         ptd::variant_index(ptd::kAdaptiveVariants, p.v) >= 0;
    printf("%s: v=%d,%d,%d spl0=%d spl=%d rounds=%u exit_skip=%d\n", name, (int)p.v.lds, p.v.sweep, (int)p.v.exit,
           p.spl0, p.spl, p.rounds, p.exit_skip);
    // the launch of the plan: every tile's parts, the sweep's or the scene's bytes of LDS
    ptd::RenderParams rp{};
    rp.spl = p.spl;
    rp.nranks = 1;
    rp.blocks_total = ((c.width + 15) / 16) * ((c.height + 15) / 16);
    rp.moments = &g_moments;
    rp.n_nodes = c.n_nodes;
    rp.n_tris = c.n_tris;
    rp.exit_skip = p.exit_skip;
    if (p.sweep) {
      rp.sweep = &g_table;
      rp.sweep_hull = p.sweep >= 2;
      rp.sweep_cube = p.sweep == 3;
      rp.sweep_boxes = c.sweep_boxes;
      rp.sweep_leaves = c.sweep_leaves;
    }
    const ptd::AdaptiveLaunch l = ptd::plan_render_adaptive(rp, p.lds);
    ok = ok && l.what == ptd::Launch::Run && l.grid == (long long)rp.blocks_total * p.spl && l.v == p.v &&
         l.lds == (p.sweep ? ptd::sweep_lds_bytes(rp) : p.lds ? ptd::scene_lds_bytes(rp) : 0);
  }
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", name);
    ++fails;
  }
}

}  // namespace

int main() {
  (void)g_list;
  const pt_adaptive_params A = {2, 9, 3, 0.25f, 0.01f};
  int rows = 0;
#define ROW(...) (row(__VA_ARGS__), ++rows)
  // ---- the instantiation ----
  ROW("box: the cube walk", box, A, {PT_OK, nullptr, 1, 3, 0, 2, 2, 3});
  ROW("box, no cube walk: the hull walk", [](pt_context* c) { box(c); c->opt_sweep_cube = 0; }, A,
      {PT_OK, nullptr, 1, 2, 0, 2, 2, 3});
  ROW("box, no hull codes: the plain sweep", [](pt_context* c) { box(c); c->opt_sweep_hull = 0; }, A,
      {PT_OK, nullptr, 1, 1, 0, 2, 2, 3});
  ROW("box, sweep off: the threaded walk in LDS", [](pt_context* c) { box(c); c->opt_small_sweep = 0; }, A,
      {PT_OK, nullptr, 1, 0, 0, 2, 2, 3});
  ROW("box from device memory: the exit skip's kernel", [](pt_context* c) { box(c); c->opt_scene_lds = 0; }, A,
      {PT_OK, nullptr, 0, 0, 1, 2, 2, 3});
  ROW("box from device memory, exit skip off", [](pt_context* c) { box(c); c->opt_scene_lds = 0; c->opt_exit_skip = 0; },
      A, {PT_OK, nullptr, 0, 0, 0, 2, 2, 3});
  ROW("a large scene: device memory, 8 lanes capped by the samples", big, A, {PT_OK, nullptr, 0, 0, 1, 2, 2, 3});
  ROW("a large scene under auto at many samples: still path-recursive", big, {64, 4096, 64, 0.25f, 0.01f},
      {PT_OK, nullptr, 0, 0, 1, 8, 8, 63});
  // ---- lanes: round 0 for min_batches, the rounds for step; never more lanes than samples ----
  ROW("lanes: min 2 step 1", box, {2, 9, 1, 0.25f, 0.01f}, {PT_OK, nullptr, 1, 3, 0, 2, 1, 7});
  ROW("lanes: min 4 step 2", box, {4, 9, 2, 0.25f, 0.01f}, {PT_OK, nullptr, 1, 3, 0, 4, 2, 3});
  ROW("lanes: min 8 step 8", box, {8, 64, 8, 0.25f, 0.01f}, {PT_OK, nullptr, 1, 3, 0, 4, 4, 7});
  ROW("lanes: the option's", [](pt_context* c) { box(c); c->opt_sample_lanes = 8; }, A,
      {PT_OK, nullptr, 1, 3, 0, 8, 8, 3});
  // ---- rounds ----
  ROW("rounds: min = max", box, {4, 4, 1, 0.25f, 0.01f}, {PT_OK, nullptr, 1, 3, 0, 4, 1, 0});
  ROW("rounds: an exact multiple", box, {2, 8, 3, 0.25f, 0.01f}, {PT_OK, nullptr, 1, 3, 0, 2, 2, 2});
  ROW("rounds: a step past the range", box, {2, 9, 100, 0.25f, 0.01f}, {PT_OK, nullptr, 1, 3, 0, 2, 4, 1});
  ROW("rounds: a step near 2^32", box, {2, 9, 0xffffffffu, 0.25f, 0.01f}, {PT_OK, nullptr, 1, 3, 0, 2, 4, 1});
  // ---- refusals ----
  const int U = PT_ERR_UNSUPPORTED, I = PT_ERR_INVALID;
  ROW("refused: the wavefront pipeline", [](pt_context* c) { box(c); c->opt_kernel = 3; }, A, {U, "PT_OPT_KERNEL 3"});
  ROW("refused: a multi-device context", [](pt_context* c) { box(c); c->group = kGroup; }, A, {U, "multi-device"});
  ROW("refused: a partition", [](pt_context* c) { box(c); c->nranks = 2; }, A, {U, "more than one rank"});
  ROW("refused: stats mode", [](pt_context* c) { box(c); c->stats_mode = true; }, A, {U, "stats mode"});
  ROW("refused: counting", [](pt_context* c) { box(c); c->opt_count = 1; }, A, {U, "PT_OPT_COUNT_TRACED"});
  ROW("refused: no moments", [](pt_context* c) { box(c); c->opt_moments = 0; }, A, {I, "PT_OPT_MOMENTS 1"});
  ROW("refused: LDS asked for a scene that cannot fit", [](pt_context* c) { big(c); c->opt_scene_lds = 2; }, A,
      {U, "too large for the LDS"});
  ROW("refused: min_batches 1", box, {1, 9, 3, 0.25f, 0.01f}, {I, "pt_adaptive_params"});
  ROW("refused: max below min", box, {4, 3, 3, 0.25f, 0.01f}, {I, "pt_adaptive_params"});
  ROW("refused: step 0", box, {2, 9, 0, 0.25f, 0.01f}, {I, "pt_adaptive_params"});
  ROW("refused: threshold 0", box, {2, 9, 3, 0.0f, 0.01f}, {I, "pt_adaptive_params"});
  ROW("refused: a NaN floor", box, {2, 9, 3, 0.25f, __builtin_nanf("")}, {I, "pt_adaptive_params"});
  ROW("refused: bad parameters come first", [](pt_context* c) { box(c); c->opt_kernel = 3; }, {1, 9, 3, 0.25f, 0.01f},
      {I, "pt_adaptive_params"});
#undef ROW
  if (fails) return 1;
  printf("ok: %d rows\n", rows);
  return 0;
}
